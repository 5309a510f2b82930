"""Seeded inputs of the SpUNet-v1m1 tests: table cases, convolution cases, state dicts, the model batch.  Used by the fixture
generator (tests/golden/make_golden_spunet.py) and by the tests, so that no weight is stored."""
import collections

import numpy as np
import torch

from ao_amd import synth

COORD_MAX = (1 << 18) - 1  # include/ptv2_spconv_hip.h: SPCONV_COORD_BITS
MARGIN = 1e-6


def lattice(counts, seed, fill=0.3):
    """clouds of `counts` distinct voxels each, drawn from ONE lattice (so that the same coordinate appears in several clouds)
    whose side makes about `fill` of the cells of the largest cloud occupied: (coord (n, 3) int32, offset (b) int32)"""
    rng = np.random.default_rng(seed)
    side = max(2, int(np.ceil((max(counts) / fill) ** (1.0 / 3.0))))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    coord = np.concatenate([cells[rng.permutation(cells.shape[0])[:c]] for c in counts]).astype(np.int32)
    return coord, np.cumsum(counts).astype(np.int32)


def _block(side, at=(0, 0, 0)):
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g + np.asarray(at)).astype(np.int32)


def table_cases():
    """{name: (coord, offset)}: the smallest inputs at which a table can go wrong"""
    cases = {}
    coord, offset = lattice((70, 9), 0)
    coord[70:74] = coord[10:14]  # four voxels of the first cloud are voxels of the second too
    assert len({tuple(v) for v in coord[70:]}) == 9
    cases["two_clouds"] = (coord, offset)
    # a voxel at coordinate 0 (neighbours at -1 and -2 are holes) and an isolated voxel far from everything
    coord, _ = lattice((40,), 1)
    coord[0] = (0, 0, 0)
    coord = np.unique(np.concatenate([coord, [[500, 500, 500]]]), axis=0).astype(np.int32)
    cases["zero_and_isolated"] = (coord[np.random.default_rng(2).permutation(coord.shape[0])], np.array([coord.shape[0]], np.int32))
    cases["full_block5"] = (_block(5, (3, 3, 3)), np.array([125], np.int32))  # the centre has every k = 5 column
    cases["one_voxel_cloud"] = (np.array([[4, 4, 4], [4, 4, 4], [5, 4, 4]], np.int32), np.array([1, 3], np.int32))
    cases["upper_bound"] = (np.array([[COORD_MAX, COORD_MAX, COORD_MAX], [COORD_MAX - 1, COORD_MAX, COORD_MAX], [0, COORD_MAX, 7]],
                                     np.int32), np.array([3], np.int32))
    # a coarse voxel with 8 children and one with 1
    cases["eight_and_one"] = (np.concatenate([_block(2, (6, 2, 4)), [[11, 9, 1]]]).astype(np.int32), np.array([9], np.int32))
    # four downsamplings that end in a single voxel: everything inside one 16^3 cell
    coord, offset = lattice((60,), 3, fill=0.02)
    assert coord.max() < 16
    cases["to_one_voxel"] = (coord + 32, offset)
    return cases


ConvCase = collections.namedtuple("ConvCase", "form cin cout k")
# (Cin, Cout, K): every width pair of the model per form; the stem
CONV_SHAPES = tuple(ConvCase("subm", *s, 27) for s in ((32, 32), (96, 96), (128, 96), (192, 128), (384, 256))) + (
    ConvCase("stem", 6, 32, 125), ConvCase("down", 32, 64, 8), ConvCase("down", 128, 256, 8),
    ConvCase("inverse", 256, 256, 8), ConvCase("inverse", 128, 96, 8))
# a ragged tail, a one-row cloud, one past a 64 boundary; many workgroups and several row splits of the weight gradient
# (3001 rows: three splits of the weight gradient)
CONV_ROWS = {"small": (70, 9), "ragged": (130, 1, 17), "many": (3001,)}


def conv_inputs(case, rows, tables_n, seed=0):
    """numpy x, weight, g_out of a convolution case; tables_n: the level sizes of the case's tables"""
    rng = np.random.default_rng(2000 + seed)
    k = round(case.k ** (1.0 / 3.0))
    n_in = tables_n[1] if case.form == "inverse" else tables_n[0]
    n_out = tables_n[1] if case.form == "down" else tables_n[0]
    x = rng.normal(0.0, 1.0, (n_in, case.cin)).astype(np.float32)
    w = (rng.uniform(-1.0, 1.0, (case.cout, k, k, k, case.cin)) / np.sqrt(case.k * case.cin)).astype(np.float32)
    g = rng.normal(0.0, 1.0, (n_out, case.cout)).astype(np.float32)
    return dict(x=x, weight=w, g_out=g)


def fill_state(shapes, seed):
    """{key: tensor} for {key: shape} in key order from numpy.random.default_rng(seed), as ptv1_cases.fill_state: convolution
    weights (Cout, k, k, k, Cin) in the default range +-1 / sqrt(k^3 Cin), biases likewise, BatchNorm weights in [0.5, 1.5],
    biases and running means N(0, 0.1), running variances in [0.5, 1.5], num_batches_tracked in [0, 5)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in shapes.items():
        stem, leaf = key.rsplit(".", 1)
        if leaf == "num_batches_tracked":
            out[key] = torch.tensor(int(rng.integers(0, 5)), dtype=torch.int64)
            continue
        if stem + ".running_mean" in shapes:
            v = rng.uniform(0.5, 1.5, shape) if leaf in ("weight", "running_var") else rng.normal(0.0, 0.1, shape)
        else:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(np.prod(shapes[stem + ".weight"][1:]))
        out[key] = torch.from_numpy(np.asarray(v, np.float32))
    return out


def shapes_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


# ---- the model batch: two synth.room_cloud clouds, grid-sampled (one row per occupied voxel, first in input order)
MODEL_CLOUDS = ((3500, 1, 0.05), (2100, 2, 0.05))  # (points, synth.room_cloud seed, voxel size in metres)
MODEL_SEED = 4  # the first seed for which no ReLU pre-activation lies within MARGIN of zero in float64 (make_golden_spunet.py --seeds)
# BasicBlock alone: same width, and 128 -> 96 with `proj`; two clouds on one lattice
BLOCK_WIDTHS = {"same": (64, 64), "proj": (128, 96)}
BLOCK_CLOUDS = (300, 41)
BLOCK_SEEDS = {"same": 0, "proj": 0}  # likewise the first with the margin


def block_inputs(form, seed=None):
    """coord, offset, x (n, Cin), g_out (n, Cout) of a block case"""
    seed = BLOCK_SEEDS[form] if seed is None else seed
    cin, cout = BLOCK_WIDTHS[form]
    coord, offset = lattice(BLOCK_CLOUDS, 50 + seed)
    rng = np.random.default_rng(3000 + seed)
    n = coord.shape[0]
    return coord, offset, rng.normal(0.0, 1.0, (n, cin)).astype(np.float32), rng.normal(0.0, 1.0, (n, cout)).astype(np.float32)


def model_batch(seed=MODEL_SEED):
    """discrete_coord, feat = (coord of the kept point, U(-1, 1)^3), segment, offset"""
    rng = np.random.default_rng(70 + seed)
    coords, feats, counts = [], [], []
    for n, cloud_seed, size in MODEL_CLOUDS:
        pts = synth.room_cloud(n, seed=cloud_seed)
        vox = np.floor((pts - pts.min(0)) / size).astype(np.int64)
        _, first = np.unique(vox, axis=0, return_index=True)
        first = np.sort(first)
        coords.append(vox[first].astype(np.int32))
        feats.append(pts[first])
        counts.append(first.shape[0])
    n = sum(counts)
    feat = np.concatenate([np.concatenate(feats), rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)], 1).astype(np.float32)
    return dict(discrete_coord=np.concatenate(coords), feat=feat, segment=rng.integers(0, 13, n).astype(np.int64),
                offset=np.cumsum(counts).astype(np.int32))
