"""Inputs of the Stratified Transformer tests: small clouds built so that every path of the kernels is taken.

window_size 0.5 and quant_size 0.125 give tables of L = 2 * 8 = 16 rows.  Every case is asserted (on the CPU, by the eager fp32
statements of tests/st_ref.py) to satisfy the reference's own asserts on the relative-position index (:153-154), for the plain
and the shifted pair lists.

  small    40 points, clouds of 25 + 15: nothing special, the smallest size
  edges    203 points, clouds of 90 + 70 + 43, every coordinate a multiple of quant_size: relative positions sit on the
           quantisation edges and points on the window edges
  dense    600 points, clouds of 420 + 180: a small window of 300 points (more than a workgroup's first pass of 256), one of
           70 (more than a wave), and a lone point whose window and large window hold nothing else: a row of one pair and a
           query without large-window keys
  long     1130 points, clouds of 1070 + 60: a small window of 1040 points, rows past the reference's cap of 1024 pairs
"""
import collections

import numpy as np

WINDOW = 0.5
QUANT = 0.125
ROWS = 16

Case = collections.namedtuple("Case", "name coords offset down_idx seed")


def _cloud(rng, n, lo, hi):
    return rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)


def _build(name):
    rng = np.random.default_rng({"small": 11, "edges": 12, "dense": 13, "long": 14}[name])
    if name == "small":
        parts = [_cloud(rng, 25, 0.0, 1.6), _cloud(rng, 15, 0.2, 1.4)]
    elif name == "edges":
        parts = [np.round(_cloud(rng, n, 0.0, 1.75) / QUANT).astype(np.float32) * np.float32(QUANT) for n in (90, 70, 43)]
    elif name == "dense":
        a = np.concatenate([_cloud(rng, 300, 0.02, 0.48), _cloud(rng, 70, 0.52, 0.98), _cloud(rng, 49, 0.0, 1.9),
                            np.array([[3.3, 3.3, 3.3]], np.float32)])
        parts = [a[rng.permutation(len(a))], _cloud(rng, 180, 0.0, 1.5)]
    elif name == "long":
        a = np.concatenate([_cloud(rng, 1040, 0.02, 0.48), _cloud(rng, 30, 0.0, 1.9)])
        parts = [a[rng.permutation(len(a))], _cloud(rng, 60, 0.0, 1.5)]
    else:
        raise KeyError(name)
    coords = np.concatenate(parts).astype(np.float32)
    offset = np.cumsum([len(p) for p in parts]).astype(np.int32)
    # the sampled points: every fourth of each cloud (unsorted on purpose), the lone point of `dense` never among them
    down = np.concatenate([np.arange(s, e, 4)[::-1] for s, e in zip(np.concatenate([[0], offset[:-1]]), offset)]).astype(np.int32)
    if name == "dense":
        lone = int(np.where((coords == np.float32(3.3)).all(1))[0][0])
        down = down[down != lone]
    return Case(name, coords, offset, down, 0)


_CASES = {}
NAMES = ("small", "edges", "dense", "long")


def case(name):
    if name not in _CASES:
        _CASES[name] = _build(name)
    return _CASES[name]


def attention_inputs(c, h, hd, rows=ROWS, seed=0):
    """q (pre-scaled), k, v, the three tables and an upstream gradient, fp32 numpy"""
    rng = np.random.default_rng(100 + seed + len(c.coords) + 7 * h + hd)
    n = len(c.coords)
    out = {k: rng.standard_normal((n, h, hd)).astype(np.float32) for k in ("q", "k", "v")}
    out["q"] *= np.float32(hd ** -0.5)
    for k in ("table_q", "table_k", "table_v"):
        out[k] = (0.5 * rng.standard_normal((rows, h, hd, 3))).astype(np.float32)
    out["g_out"] = rng.standard_normal((n, h * hd)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------ the model ----
# the small configuration of the model tests: every head has 16 channels, two levels of two blocks (a plain and a shifted one)
MODEL_CONFIG = dict(in_channels=6, num_classes=13, channels=(16, 32, 32), num_heads=(2, 2), depths=(2, 2), window_size=(1.0, 2.0),
                    quant_size=(0.25, 0.5), down_num_sample=8, kp_ball_radius=0.5, kp_max_neighbor=8, kp_grid_size=0.2,
                    drop_path_rate=0.0)
# clouds of unequal size.  In the three-cloud batch the quarter shares of the second and third cloud end in .5 and .5: the
# accumulated float of TransitionDown (:449-455) reaches 76 where the per-cloud truncation of BasicLayer (:340-346) gives 75
MODEL_CLOUDS = {"st2": (150, 90), "st3": (120, 70, 102)}
# the first seed of each batch for which the reference's asserts hold and the relative-position index of every block is the same
# whether a division by a python scalar divides (CPU) or multiplies by the fp32 reciprocal (GPU): make_golden_st.py --seeds
MODEL_SEEDS = {"st2": 0, "st3": 0}
STATE_SEED = 7
SMALL_PARAMETER = 4096


def model_batch(name, seed=None):
    rng = np.random.default_rng(1000 + (MODEL_SEEDS[name] if seed is None else seed) + 17 * len(MODEL_CLOUDS[name]))
    sizes = MODEL_CLOUDS[name]
    coord = np.concatenate([rng.uniform(0.0, 2.0, (n, 3)) for n in sizes]).astype(np.float32)
    feat = np.concatenate([coord / 2.0, rng.uniform(0.0, 1.0, (len(coord), 3))], 1).astype(np.float32)
    segment = rng.integers(0, 13, len(coord)).astype(np.int64)
    return dict(coord=coord, feat=feat, offset=np.cumsum(sizes).astype(np.int32), segment=segment)


def fill_state(shapes, seed=STATE_SEED):
    """{key: numpy fp32 array} for {key: shape}, in key order from one generator.  Linear weights +-1/sqrt(fan_in); norm weights
    in [0.5, 1.5]; biases and running means N(0, 0.1); running variances in [0.5, 1.5]; the three relative-position tables
    N(0, 0.2) (the reference leaves two of them at zero); KPConv weights N(0, 1/sqrt(15 cin)).  K_points keeps its
    deterministic initial value and num_batches_tracked its zero: they are not in the result."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in shapes.items():
        stem, leaf = key.rsplit(".", 1)
        if leaf in ("K_points", "num_batches_tracked"):
            continue
        if leaf.startswith("relative_pos_"):
            v = rng.normal(0.0, 0.2, shape)
        elif stem.endswith("kpconv"):
            v = rng.normal(0.0, 1.0, shape) / np.sqrt(15 * shape[1])
        elif leaf == "running_var" or (leaf == "weight" and len(shape) == 1):
            v = rng.uniform(0.5, 1.5, shape)
        elif leaf in ("bias", "running_mean"):
            v = rng.normal(0.0, 0.1, shape)
        else:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shape[1])
        out[key] = np.asarray(v, np.float32)
    return out
