"""GPU: the bf16-operand form of OctFormer's octree convolutions (ao_amd/csrc/oct_conv_bf16.hip through operands="bf16" of
ao_amd.octformer.octree_conv) and OctFormer(conv_operands="bf16"), on the cases of tests/octconv_cases.py without the stem's.

Exact: x, g and bias integers in [-4, 4], weights from {-1, -1/2, 0, 1/2, 1}: every operand is a bf16 value and every partial sum
a multiple of 1/2 far below 2^24 (27 * 384 * 4 = 41 472; 245 rows * 16), so fp32 accumulation in any order is exact and y, g_x,
g_w, g_b must EQUAL the float64 run of octree_conv_torch: no wrong lane, pitch, transpose, reverse, tail chunk or skipped -1 passes.
Rounded random: C.layer_inputs against tests/octconv_ref.py in float64 on x, weights and g rounded through .bfloat16(), by the
rule of tests/test_gpu_octconv.py: e_kernel <= M[key] max(e_eager, 2^-24) in relative L2, e_eager the fp32 run of the reference on
the same rounded operands.  The op takes the unrounded operands on both paths; the eager path rounds no gradient, so it alone is
handed the rounded g.  g_b has no matrix operand: the HIP path's is held to the column sums of the unrounded g it was given.
Model: the HIP run's distance from the UNROUNDED float64 run is at most M["model"] times the AO_AMD_OCTFORMER=torch bf16 run's.
M: twice the worst ratio measured on the MI355X, rounded up to a power of two, in [1, 64]; every ratio is
printed as an `octconv-bf16-ratio` line."""
import copy

import numpy as np
import pytest
import torch

from tests import octconv_cases as C
from tests import octconv_ref as R
from tests import test_gpu_octconv as T   # its _dev(), _l2(), pyramid(), model_run(), MODEL_KEYS and FLOOR; none of its tests

pytestmark = pytest.mark.gpu

CASES = [c for c in C.CASES if c[1] != 6]
IDS = ["%s-%d-%d-%s" % (c[0], c[1], c[2], c[4]) for c in CASES]
KEYS = ("y", "g_x", "g_w", "g_b")
# worst ratios measured: y 1.227 (conv3 168 -> 168), g_x 1.477 (deconv3 16 -> 24, block), g_w 1.000, g_b 1.590; model 1.003
M = {"y": 4, "g_x": 4, "g_w": 2, "g_b": 4, "model": 4}
_REF = {}


def _run(t, fn, dtype, g=None):
    x, w, b = (None if t[k] is None else T._dev(t[k]).to(dtype).requires_grad_(True) for k in ("x", "weights", "bias"))
    y = fn(x, w, b)
    grads = torch.autograd.grad(y, [v for v in (x, w, b) if v is not None], T._dev(t["g"] if g is None else g).to(dtype))
    return dict(zip(KEYS, (y.detach(),) + grads))


def _ours(case, t, operands="bf16", g=None):
    from ao_amd.octformer import octree_conv

    p = T.pyramid(case[4])
    table = p.level(C.DEPTH) if case[0] == "conv3" else p.link(C.DEPTH)
    return _run(t, lambda x, w, b: octree_conv(x, w, b, table, case[0], operands=operands), torch.float32, g)


def _exact(t):
    """the operands of `t` redrawn as small bf16 values: integers in [-4, 4], weights from {-1, -1/2, 0, 1/2, 1}"""
    gen = torch.Generator().manual_seed(7)
    ints = lambda a: None if a is None else torch.randint(-4, 5, a.shape, generator=gen).float()   # noqa: E731
    return dict(t, x=ints(t["x"]), g=ints(t["g"]), bias=ints(t["bias"]),
                weights=torch.randint(-2, 3, t["weights"].shape, generator=gen).float() * 0.5)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_on_bf16_valued_inputs(case, monkeypatch):
    from ao_amd.octformer import octree_conv_torch

    monkeypatch.setenv("AO_AMD_OCTFORMER", "hip")
    t = _exact(C.layer_inputs(*case))
    want = _run(t, lambda x, w, b: octree_conv_torch(x, w, b, T._dev(t["tab"]), t["transpose"]), torch.float64)
    got = _ours(case, t)
    assert set(got) == set(want) == set(KEYS[:3 + case[3]])
    for key in got:
        assert got[key].dtype == torch.float32 and torch.equal(got[key], want[key].float()), key


def test_exact_across_the_row_splits_of_the_weight_gradient(monkeypatch):
    """a full 12 x 12 x 12 block, 1728 rows with every slot present: two row splits (896 + 832 rows, the second with a tail
    stage) and the finalize, which the 245-row cases never reach; 1728 * 16 is still far below 2^24"""
    from ao_amd.octformer import octree_conv, octree_conv_torch, octree_pyramid

    monkeypatch.setenv("AO_AMD_OCTFORMER", "hip")
    xyz = np.stack(np.meshgrid(*[np.arange(100, 112)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    level = octree_pyramid(T._dev(xyz), T._dev(np.zeros(len(xyz), np.int64)), C.DEPTH, 2).level(C.DEPTH)
    t = _exact(dict(x=np.empty((level.n, 48)), weights=np.empty((27, 48, 48)), bias=None, g=np.empty((level.n, 48))))
    want = _run(t, lambda x, w, b: octree_conv_torch(x, w, b, level.nbr, False), torch.float64)
    got = _run(t, lambda x, w, b: octree_conv(x, w, b, level, "conv3", operands="bf16"), torch.float32)
    assert level.n == 1728 and all(torch.equal(got[k], want[k].float()) for k in want)


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounded_random_against_float64(case, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_OCTFORMER", path)
    if case not in _REF:   # (once for both paths)
        raw = C.layer_inputs(*case)
        rounded = dict(raw, **{k: torch.from_numpy(raw[k]).bfloat16().float() for k in ("x", "weights", "g")})
        fn = lambda x, w, b: R.conv(x, w, b, T._dev(raw["tab"]), raw["transpose"])   # noqa: E731
        _REF.clear()
        _REF[case] = (raw, rounded, _run(rounded, fn, torch.float64), _run(rounded, fn, torch.float32))
    raw, rounded, f64, f32 = _REF[case]
    got = _ours(case, raw, g=rounded["g"] if path == "torch" else None)
    if path == "hip" and case[3]:   # the bias gradient has no matrix operand: the kernels add the unrounded g they were given
        f64, f32 = dict(f64, g_b=T._dev(raw["g"]).double().sum(0)), dict(f32, g_b=T._dev(raw["g"]).sum(0))
    bad = []
    for key in sorted(f64):
        assert got[key].dtype == torch.float32 and torch.isfinite(got[key]).all(), key
        e, eager = T._l2(got[key], f64[key]), max(T._l2(f32[key], f64[key]), T.FLOOR)
        print("octconv-bf16-ratio %-28s %-5s %-4s kernel %.3e eager %.3e ratio %.3f" % (IDS[CASES.index(case)], path, key, e, eager, e / eager))
        if not e <= M[key] * eager:
            bad.append((key, e, eager))
    assert not bad, bad


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]], ids=lambda c: c[0])
def test_two_runs_give_the_same_bits(case, monkeypatch):
    monkeypatch.setenv("AO_AMD_OCTFORMER", "hip")
    t = C.layer_inputs(*case)
    a, b = _ours(case, t), _ours(case, t)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_operands_keyword(monkeypatch):
    monkeypatch.setenv("AO_AMD_OCTFORMER", "hip")
    case, stem = CASES[0], C.CASES[0]
    t, s = C.layer_inputs(*case), C.layer_inputs(*stem)
    fp32, bf16 = _ours(case, t, "fp32"), _ours(case, t, "bf16")
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)   # noqa: E731
    assert not torch.equal(fp32["y"], bf16["y"]) and same(_ours(case, t, "autocast"), fp32)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = _ours(case, t, "autocast")
        assert same(_ours(case, t, "fp32"), fp32)
    assert cast["y"].dtype == torch.float32 and same(cast, bf16)
    assert stem[1] == 6 and same(_ours(stem, s, "bf16"), _ours(stem, s, "fp32"))   # the stem keeps its fp32 kernel
    with pytest.raises(ValueError, match="operands"):
        _ours(case, t, "nope")


def test_octformer_with_bf16_operands(monkeypatch):
    from ao_amd.octformer import OctFormer

    xyz, batch = C.OC.cloud((150, 150), seed=11)
    rng = np.random.default_rng(11)
    coord = ((xyz + 0.5) / 256.0 - 1.0) * 10.24
    data = dict(coord=T._dev(coord.astype(np.float32)), normal=None, feat=T._dev(rng.standard_normal((300, 6)).astype(np.float32)),
                offset=T._dev(np.cumsum(np.bincount(batch))))
    g = T._dev(rng.standard_normal((300, 5)).astype(np.float32))
    torch.manual_seed(11)
    model = OctFormer(in_channels=6, num_classes=5, fpn_channels=24, channels=(32, 64), num_blocks=(1, 1), num_heads=(2, 4),
                      patch_size=8, dilation=2, stem_down=2, head_up=2, drop_path=0.0, octree_depth=7, octree_full_depth=2,
                      conv_operands="bf16").cuda().train()
    monkeypatch.setenv("AO_AMD_OCTFORMER", "hip")
    res = T.model_run(copy.deepcopy(model), data, g)
    monkeypatch.setenv("AO_AMD_OCTFORMER", "torch")
    eager = T.model_run(copy.deepcopy(model), data, g)
    f64 = T.model_run(copy.deepcopy(model).double(), data, g)   # float64 operands are not rounded
    bad = []
    for key in sorted(T.MODEL_KEYS):
        assert torch.isfinite(res[key]).all(), key
        e, ref = T._l2(res[key], f64[key]), T._l2(eager[key], f64[key])
        print("octconv-bf16-ratio model %-36s hip %.3e torch %.3e ratio %.3f" % (key, e, ref, e / ref))
        if not e <= M["model"] * ref:
            bad.append((key, e, ref))
    assert not bad, bad
