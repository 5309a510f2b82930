"""Seeded inputs of the Point Transformer V1 tests: state dicts, layer cases, the model batch.  Used by the fixture generator
(tests/golden/make_golden_ptv1.py) and by the tests, so that no weight is stored."""
import collections

import numpy as np
import torch

from ao_amd import synth

LayerCase = collections.namedtuple("LayerCase", "name c ns clouds seed")
# (C, ns, clouds): every level width; a ragged tail, a one-point cloud (15 invalid slots in a row), clouds shorter than ns
# (-1 slots inside the softmax and all three norms), one past a 64-point boundary, the largest weight (64 x 512: two channels
# per thread, eight channel chunks in the weight-gradient pass, the smallest record grids), many workgroups.
# The seeds are the first for which no ReLU pre-activation behind a norm lies within MARGIN of its kink in float64
# (tests/golden/make_golden_ptv1.py --seeds finds them): nearer, fp32 rounding decides the mask and a gradient is not continuous
LAYER_CASES = (
    LayerCase("c32", 32, 8, (70, 9), 0),
    LayerCase("c64", 64, 16, (130, 1, 17), 0),
    LayerCase("c128", 128, 16, (12, 5, 40), 1),
    LayerCase("c256", 256, 16, (65,), 0),
    LayerCase("c512", 512, 16, (33, 7), 0),
    LayerCase("many", 64, 16, (3001,), 15),
)
EVAL_CASES = ("c32", "c128")
GOLDEN_LAYER_CASES = ("c32", "c128")
MARGIN = 1e-6
MODEL_SEED = 11
MODEL_CLOUDS = ((2100, 0), (1300, 1))  # (points, synth.room_cloud seed)
LEVEL_SHAPES = ((80000, 8, 32), (20000, 16, 64), (5000, 16, 128), (1250, 16, 256), (312, 16, 512))


def case(name):
    return {c.name: c for c in LAYER_CASES}[name]


def fill_state(shapes, seed):
    """{key: tensor} for {key: shape} in key order from numpy.random.default_rng(seed): Linear weights and biases in the
    default range +-1/sqrt(fan_in), BatchNorm weights in [0.5, 1.5], biases and running means N(0, 0.1), running variances in
    [0.5, 1.5], num_batches_tracked in [0, 5)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in shapes.items():
        stem, leaf = key.rsplit(".", 1)
        norm = stem + ".running_mean" in shapes
        if leaf == "num_batches_tracked":
            out[key] = torch.tensor(int(rng.integers(0, 5)), dtype=torch.int64)
            continue
        if norm:
            if leaf in ("weight", "running_var"):
                v = rng.uniform(0.5, 1.5, shape)
            else:
                v = rng.normal(0.0, 0.1, shape)
        else:
            fan_in = shapes[stem + ".weight"][1]
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)
        out[key] = torch.from_numpy(np.asarray(v, np.float32))
    return out


def shapes_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def self_knn(coord, clouds, ns):
    """the self-kNN table of the clouds, -1 where a cloud has fewer than ns points (brute force, ties by index)"""
    idx = np.full((coord.shape[0], ns), -1, np.int32)
    start = 0
    for cnt in clouds:
        c = coord[start:start + cnt].astype(np.float64)
        d = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")[:, :ns]
        idx[start:start + cnt, :order.shape[1]] = order + start
        start += cnt
    return idx


def layer_state(module, c, seed=None):
    """the seeded state dict of a layer case for a module with the layer's keys"""
    return fill_state(shapes_of(module), 100 + (c.seed if seed is None else seed))


def layer_inputs(c, seed=None):
    """numpy inputs of a layer case: coord, idx, x_q, x_k, x_v, g_out"""
    rng = np.random.default_rng(1000 + (c.seed if seed is None else seed))
    n = sum(c.clouds)
    coord = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    out = dict(coord=coord, idx=self_knn(coord, c.clouds, c.ns))
    for key in ("x_q", "x_k", "x_v", "g_out"):
        out[key] = rng.normal(0.0, 1.0, (n, c.c)).astype(np.float32)
    return out


def model_batch():
    """the two-cloud batch of the model fixture: coord, feat = (coord, U(-1, 1)^3), segment, offset"""
    rng = np.random.default_rng(7)
    coord = np.concatenate([synth.room_cloud(n, seed=s) for n, s in MODEL_CLOUDS]).astype(np.float32)
    n = coord.shape[0]
    feat = np.concatenate([coord, rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)], 1)
    segment = rng.integers(0, 13, n).astype(np.int64)
    offset = np.cumsum([c for c, _ in MODEL_CLOUDS]).astype(np.int32)
    return dict(coord=coord, feat=feat, segment=segment, offset=offset)
