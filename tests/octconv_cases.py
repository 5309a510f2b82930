"""Cases of the octree convolution tests: the clouds of tests/octformer_cases.py at depth 9 with their dictionary-built tables."""
import functools

import numpy as np

from tests import octconv_ref as R
from tests import octformer_cases as OC

DEPTH = OC.DEPTH
# 245 child rows: three full 64-row tiles and a tail, a tile across the cloud boundary, a dense blob (parents with several
# children; up rows with 1, 2, 3 and 4 entries: none of its nodes has all 8 candidate parents) | less than one 16-row matrix
# tile | a full 4 x 4 x 4 block at 10 .. 13: every parent has 8 children, the all-odd nodes have up rows of 8
CLOUDS = {"two-clouds": ((100, 145), 7), "tiny": ((19,), 1), "block": None}
# (form, Cin, Cout, bias, cloud): every pair on two-clouds, the narrowest of each form on tiny too.  (16, 24) of the deconv is
# the unequal pair that catches a transposed weight read; 6 is the stem's zero-padded contraction; 168 = 10.5 column tiles
LAYERS = [("conv3", 6, 24, False), ("conv3", 48, 48, False), ("conv3", 168, 168, False), ("down2", 24, 48, True),
          ("down2", 96, 192, True), ("deconv3", 168, 168, False), ("deconv3", 16, 24, False)]
CASES = [c + ("two-clouds",) for c in LAYERS] + [LAYERS[0] + ("tiny",), LAYERS[3] + ("tiny",), LAYERS[6] + ("tiny",), LAYERS[6] + ("block",)]


@functools.lru_cache(None)
def tables(name):
    if name == "block":
        xyz = np.stack(np.meshgrid(*[np.arange(10, 14)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
        xyz, batch = xyz[np.argsort(OC.morton(xyz[:, 0], xyz[:, 1], xyz[:, 2]))], np.zeros(64, np.int64)
    else:
        xyz, batch = OC.cloud(CLOUDS[name][0], seed=CLOUDS[name][1])
    t = dict(R.hierarchy(xyz, batch), xyz=xyz, batch=batch, nbr=R.dict_neighbours(xyz, batch))
    if name == "two-clouds":
        assert (np.bincount(t["parent"]) > 1).sum() >= 8, "parents with several children"
        assert {1, 2, 3, 4} <= set((t["up"] >= 0).sum(1).tolist()), "up rows of several sizes"
    if name == "block":
        assert {1, 2, 4, 8} == set((t["up"] >= 0).sum(1).tolist()) and (np.bincount(t["parent"]) == 8).all()
    return t


def layer_inputs(form, cin, cout, bias, name):
    """numpy operands of one case: x, weights, bias or None, the output's gradient, the forward table and its transpose flag"""
    t = tables(name)
    n, m = len(t["xyz"]), len(t["pxyz"])
    tab, n_in, transpose = {"conv3": (t["nbr"], n, False), "down2": (t["child"], n, False), "deconv3": (t["up"], m, True)}[form]
    rng = np.random.default_rng(1000 * cin + cout)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(x=f(n_in, cin), weights=f(tab.shape[1], *((cout, cin) if transpose else (cin, cout))), bias=f(cout) if bias else None,
                g=f(len(tab), cout), tab=tab, transpose=transpose)
