"""Inputs of tests/test_gpu_cac_f64.py and tests/test_cac_ref64_host.py, built on the CPU from fixed seeds.

Every case comes in two value tiers: *plain* (logits ~ N(0, 3^2), features ~ N(0, 2^2)) and *wide* (logits x 30: a softmax
without the max subtraction overflows; features +-10^U(-3, 3)).  The builder keeps every discontinuity of a contract away from
rounding and asserts it in float64:

* a masked case has |max_k p_nk - thr| >= 1e-3 in every row and rows on both sides of thr;
* class counts are integers (mode 1's z, the distillation's rows): nothing rounds across `> 0`;
* the distillation's 1 / (sum_n ent_n + 1e-4) has a pole: |den_k + 1e-4| >= 2^-6 (sum_n |ent_n| + 1e-4) for every present class.
  With K = 1 the softmax is 1, ent_n = -log(1.0001) and ONE labelled row sits on that pole (den + 1e-4 = 5e-9): K = 1 runs with
  256 and 257 rows, and with one ignored row.  The wide tier's `soft` rows keep a runner-up within 2 of the maximum, or every
  row's entropy is -1e-4 and every class with one row sits there too.

Scene cases (weighted sums and cosine logits) are (K, C) x row layout; the pairs and layouts are the smallest that reach each
path of ao_amd/csrc/cac.hip (TILE 16, COS_TILE 64, CHUNK 256, the second 64-lane slot of a row at K = 65, one class group per
workgroup at K = 200, the full accumulator table at K = 256, C = 64, 2305 rows = ten slabs for the eight-chain finalize loop and its tail)."""
import zlib
from collections import namedtuple

import numpy as np

from tests import cac_ref64 as R

F32, F64 = np.float32, np.float64
TIERS = ("plain", "wide")
Case = namedtuple("Case", "name family p flags")

PROTO_EPS, MEAN_EPS, COS_SCALE = 1e-7, 1e-4, 15.0     # ao_amd/ptv2/cac.py; cos_temp of the CAC configs
THR_MARGIN, POLE_MARGIN = 1e-3, 2.0 ** -6

LAYOUTS = dict(r1=(1,), r15=(15,), r16=(16,), r17=(17,), r63=(63,), r64=(64,), r65=(65,), r255=(255,), r256=(256,), r257=(257,),
               s300_0_17=(300, 0, 17), r2305=(2305,), s3x1000=(1000, 990, 1010))
SCENE_GRID = (
    (20, 48, tuple(LAYOUTS)),
    (1, 4, ("r1", "r17", "s300_0_17")),
    (64, 8, ("r65", "r257")),
    (65, 8, ("r16", "r257", "r2305", "s3x1000")),
    (200, 48, ("r17", "r257", "s300_0_17")),
    (256, 64, ("r1", "r64", "r257")),
)


def _scene_cases():
    out = []
    for k, c, layouts in SCENE_GRID:
        for lay in layouts:
            n = sum(LAYOUTS[lay])
            thr = 0.75 if k >= 20 and n >= 15 and (k, lay) != (20, "r257") and k != 65 else 0.0
            out.append(Case("k%d-c%d-%s-thr%s" % (k, c, lay, "075" if thr else "0"), "scene",
                            dict(k=k, c=c, sizes=LAYOUTS[lay], thr=thr), ()))
    out.append(Case("k20-c48-r257-thr0-zeros", "scene", dict(k=20, c=48, sizes=(257,), thr=0.0), ("zeros",)))
    return out


DISTILL_GRID = ((20, 1, "all"), (20, 255, "all"), (20, 256, "all"), (20, 257, "all"), (20, 16385, "all"), (20, 257, "ign30"),
                (20, 257, "absent"), (20, 257, "allign"), (20, 16385, "ign30"), (1, 257, "all"), (1, 256, "ign30"),
                (1, 1, "allign"), (65, 1, "all"), (65, 257, "ign30"), (65, 255, "absent"), (65, 16385, "ign30"),
                (200, 257, "ign30"), (200, 1, "allign"), (256, 257, "all"), (256, 255, "absent"), (256, 256, "ign30"))
# (c, n, ignored fraction, ignore_index, flags)
CE_GRID = ((1, 1, 0.0, -1, ()), (1, 257, 0.1, 255, ()), (2, 1, 0.0, 255, ()), (2, 257, 0.1, -1, ()), (13, 1, 1.0, -1, ()),
           (13, 257, 0.0, -1, ()), (13, 257, 0.1, 255, ()), (13, 257, 1.0, 255, ()), (64, 1, 0.0, -1, ()), (64, 257, 0.1, -1, ()),
           (64, 257, 0.0, 255, ()), (13, 257, 0.1, -1, ("bad",)),
           (13, 262144 + 257, 0.1, -1, ("stride",)),      # above 1024 x 256 rows: the forward's grid-stride loop
           (2, 1048576 + 257, 0.1, -1, ("stride",)))      # above 4096 x 256 rows: the backward's (8 MB of logits)

CASES = dict(
    scene=_scene_cases(),
    distill=[Case("k%d-n%d-%s" % g, "distill", dict(k=g[0], n=g[1], layout=g[2]), ()) for g in DISTILL_GRID],
    ce=[Case("c%d-n%d-ig%g-ii%d%s" % (c, n, f, ii, "".join("-" + x for x in fl)), "ce", dict(c=c, n=n, frac=f, ignore_index=ii), fl)
        for c, n, f, ii, fl in CE_GRID],
)
FAMILY = dict(
    cac_weighted_sum_forward_hip_launcher="scene", cac_weighted_sum_backward_hip_launcher="scene",
    cac_cosine_forward_hip_launcher="scene", cac_cosine_backward_hip_launcher="scene",
    cac_distill_forward_hip_launcher="distill", cac_distill_backward_hip_launcher="distill",
    cross_entropy_forward_hip_launcher="ce", cross_entropy_backward_hip_launcher="ce",
)


def pairs(family, stride=True):
    return [(c, t) for c in CASES[family] for t in TIERS if stride or "stride" not in c.flags]


def _rng(case, tier):
    return np.random.default_rng(zlib.crc32(("%s/%s/%s" % (case.family, case.name, tier)).encode()))


def _features(rng, shape, tier, sigma=2.0):
    if tier == "plain":
        return (rng.standard_normal(shape) * sigma).astype(F32)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F32)


def _softmax64(l):
    e = np.exp(l.astype(F64) - l.astype(F64).max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _logits(rng, n, k, tier, thr):
    l = (rng.standard_normal((n, k)) * 3.0).astype(F32)
    if thr > 0:
        order, rows = np.argsort(l, 1), np.arange(n)
        top, second = order[:, -1], order[:, -2]
        up, down = rows % 7 == 0, rows % 7 == 1
        l[rows[up], top[up]] += F32(20.0)                       # above thr
        l[rows[down], second[down]] = l[rows[down], top[down]]  # a tie: max p <= 0.5, below thr
    if tier == "wide":
        l = l * F32(30.0)
    if thr > 0:
        for _ in range(64):   # rows whose max p is within the margin of thr move away from it
            near = np.abs(_softmax64(l).max(1) - thr) < 2 * THR_MARGIN
            if not near.any():
                break
            l[near, l[near].argmax(1)] += F32(1.0 if tier == "plain" else 30.0)
        top = _softmax64(l).max(1)
        assert (np.abs(top - thr) >= THR_MARGIN).all() and (top > thr).any() and (top < thr).any()
    return l


_CACHE = {}


def inputs(case, tier):
    """the numpy inputs of a case, built once (read-only: they are shared)"""
    key = (case.family, case.name, tier)
    if key not in _CACHE:
        _CACHE[key] = _build(case, tier)
    return _CACHE[key]


def _build(case, tier):
    rng, p = _rng(case, tier), case.p
    if case.family == "scene":
        k, c, sizes = p["k"], p["c"], p["sizes"]
        n, b = sum(sizes), len(sizes)
        x = _features(rng, (n, c), tier)
        label = rng.integers(0, k, n)
        if k >= 20:
            label[np.isin(label, (3, 7))] = 5                   # two classes absent
        if n >= 15:
            label[rng.random(n) < 0.1] = -1
            label[1] = -1
        q = _features(rng, (b, k, c), tier, 1.0)
        if "zeros" in case.flags:
            x[5], q[:, 2] = 0, 0
        t = dict(k=k, c=c, n=n, b=b, x=x, logits=_logits(rng, n, k, tier, p["thr"]), label=label.astype(np.int64),
                 offset=np.cumsum(sizes).astype(np.int32), max_rows=max(sizes), thr=p["thr"], q=q,
                 dout_sets=rng.standard_normal((b, k, c)).astype(F32), dout_rows=rng.standard_normal((n, k)).astype(F32))
        assert (np.bincount(label[label >= 0], minlength=k) < 2 ** 24).all()
        return t
    if case.family == "distill":
        k, n, layout = p["k"], p["n"], p["layout"]
        pred, soft = (rng.standard_normal((n, k)) * 3.0).astype(F32), (rng.standard_normal((n, k)) * 3.0).astype(F32)
        if tier == "wide":
            pred, soft = pred * F32(30.0), soft * F32(30.0)
            if k > 1:
                order, rows = np.argsort(soft, 1), np.arange(n)
                soft[rows, order[:, -2]] = soft[rows, order[:, -1]] - rng.uniform(0, 2, n).astype(F32)
        label = rng.integers(0, k, n)
        if layout == "ign30":
            label[rng.random(n) < 0.3] = -1
            label[0] = -1
        elif layout == "absent":
            label[label == k // 2] = (k // 2 + 1) % k
        elif layout == "allign":
            label[:] = -1
        if layout != "allign":
            label[-1] = k - 1      # the last class (the second lane slot of a row at K = 65) carries a one-hot half
        t = dict(k=k, n=n, pred=pred, soft=soft, label=label.astype(np.int64), g=2.5)
        _, _, _, _, ent, g, _ = R._distill(t, F64, None)
        den, present = R.rowsum(ent, g), np.bincount(label[label >= 0], minlength=k) > 0
        assert (np.abs(den.v + 1e-4) >= POLE_MARGIN * (den.a + 1e-4))[present].all(), (case.name, tier)
        assert present.any() == (layout != "allign") and (layout != "absent" or not present.all())
        return t
    c, n, frac, ii = p["c"], p["n"], p["frac"], p["ignore_index"]
    logits = (rng.standard_normal((n, c)) * 3.0).astype(F32) * F32(30.0 if tier == "wide" else 1.0)
    label = rng.integers(0, c, n)
    if frac >= 1.0:
        label[:] = ii
    elif frac > 0:
        label[rng.random(n) < frac] = ii
        label[n // 2] = ii
    if "bad" in case.flags:
        label[n // 3] = c          # neither ignore_index nor in [0, c)
    return dict(c=c, n=n, logits=logits, label=label.astype(np.int64), ignore_index=ii, g=1.7)


def view(case, tier, launcher, mode=0, per_scene=1, glogits=True):
    """the dict a statement of tests/cac_ref64.py takes for `launcher` on this case"""
    t = inputs(case, tier)
    if "weighted_sum" in launcher:
        return dict(mode=mode, k=t["k"], x=t["x"], logits=t["logits"], label=t["label"], offset=t["offset"],
                    thr=t["thr"] if mode == 0 else 0.0, eps=PROTO_EPS if mode == 0 else MEAN_EPS,
                    dout=t["dout_sets"] if mode == 0 else t["dout_sets"][:1], glogits=glogits and mode == 0)
    if "cosine" in launcher:
        return dict(k=t["k"], x=t["x"], q=t["q"] if per_scene else t["q"][0], per_scene=per_scene, offset=t["offset"],
                    scale=COS_SCALE, dout=t["dout_rows"])
    return t


def variants(case, launcher):
    """the (mode, per_scene, glogits) settings a scene launcher runs a case in"""
    if "weighted_sum_forward" in launcher:
        return [dict(mode=0), dict(mode=1)]
    if "weighted_sum_backward" in launcher:   # glogits absent: on the smallest, a tile-edge and the multi-scene layout
        absent = case.p.get("sizes") in ((1,), (17,), (300, 0, 17))
        return [dict(mode=0), dict(mode=1)] + ([dict(mode=0, glogits=False)] if absent else [])
    if "cosine" in launcher:                  # per-scene prototypes; shared ones where there is more than one scene, and once at 257
        shared = len(case.p["sizes"]) > 1 or case.p["sizes"] == (257,)
        return [dict(per_scene=1)] + ([dict(per_scene=0)] if shared else [])
    return [dict()]


def reference(case, tier, launcher, **variant):
    """the float64 statement of `launcher` on the case: computed once, shared by the tests (read-only)"""
    key = (case.family, case.name, tier, launcher, tuple(sorted(variant.items())))
    if key not in _CACHE:
        _CACHE[key] = R.CONTRACTS[launcher](view(case, tier, launcher, **variant))
    return _CACHE[key]
