"""GPU: ao_amd.swin3d's half-precision path (fp16_mode 1; ao_amd/csrc/swin_attention_f16.hip).

Against float64: crse_attention on qkv.half(), g_out.half(), fp32 tables, fp16_mode=1, for every case of tests/swin3d_cases.py,
against tests/swin3d_ref.py in float64 on qkv.half() and table.half() -- the values the kernels read.  The rule is that of
tests/test_gpu_swin3d_ops.py, e_kernel <= M[key] * max(e_eager, floor) in relative L2, with e_eager the fp32 run of the same
reference with out and g_qkv rounded to half, floor = 2^-11 (half's unit roundoff) for the half-stored keys and 2^-24 for the
table gradients.  M per key: twice the worst ratio measured on the MI355X over the six cases, rounded up to a power of two
(DESIGN.md section 22 holds the table).

The M of g_q_table and g_k_table is NOT a small number and is a finding, not a tolerance to rely on: both gradients are sums of
dS = P (dP - delta), and delta = g_out . out is formed from the half-rounded out the forward saved, so they carry half's
roundoff (their e_kernel is 3.1e-4 .. 6.8e-4, about 2^-11, on the five cases with real windows) while the rule measures them
against an fp32 e_eager of 2e-7 .. 1e-6: worst ratios 13947 and 13765 on single-member (e_kernel 3.2e-3, 3.3e-3), where 196
windows of one voxel have dS = 0 exactly in the reference and only four small windows carry the gradient.  g_v_table, which
depends on P alone, stays at 2.36.

The layer test runs a BasicLayer(fp16_mode=1) under fp16 autocast against the same module under AO_AMD_SWIN3D=torch and the same
autocast: both run the same half Linears and differ in the attention alone, whose results each path rounds to half once, so the
distance is measured in units of 2^-11; M the same way."""
import numpy as np
import pytest
import torch

from tests import swin3d_cases as SC
from tests import swin3d_ref as R

pytestmark = pytest.mark.gpu

HALF_KEYS = ("out", "g_qkv")
KEYS = {"out", "g_qkv", "g_q_table", "g_k_table", "g_v_table"}
FLOOR = {k: 2.0 ** (-11 if k in HALF_KEYS else -24) for k in KEYS}
# M per key: 2 x the worst e_kernel / max(e_eager, floor) over every case, as a power of two
M = {"out": 1, "g_qkv": 8, "g_q_table": 32768, "g_k_table": 32768, "g_v_table": 8}
# the layer: 2 x the worst distance / 2^-11, as a power of two (at least 1); "g_param" is shared by the parameter gradients
M_LAYER = {"out": 1, "g_feats": 4, "g_param": 4}

_REF = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def run(name, fn, dtype, qkv_dtype=None, half_tables=False):
    """out and the four gradients of fn; qkv is a leaf of `qkv_dtype` holding half values, the tables are leaves of `dtype`
    holding the fp32 values or, with half_tables, the half values a workgroup stages"""
    _, _, H, hd, _, _, _ = SC.CASES[name]
    t = SC.attention_inputs(name)
    qkv = _dev(t["qkv"]).half().to(qkv_dtype or dtype).requires_grad_(True)
    tq, tk, tv = ((_dev(t[k]).half() if half_tables else _dev(t[k])).to(dtype).requires_grad_(True) for k in ("q_table", "k_table", "v_table"))
    out = fn(t, qkv, tq, tk, tv, SC.table_rows(name), hd ** -0.5, H)
    grads = torch.autograd.grad(out, (qkv, tq, tk, tv), _dev(t["g_out"]).half().to(out.dtype))
    return dict(zip(("out", "g_qkv", "g_q_table", "g_k_table", "g_v_table"), (out.detach(),) + grads))


def reference(name):
    """(float64, fp32 with out and g_qkv rounded to half) of the reference statements on the half-rounded tables"""
    if name not in _REF:
        def fn(t, qkv, tq, tk, tv, rows, s, H):
            return R.attention(qkv, t["parts"], _dev(t["signals"]), tq, tk, tv, rows, s, H)

        f64, f32 = (run(name, fn, dt, half_tables=True) for dt in (torch.float64, torch.float32))
        f32.update({k: f32[k].half() for k in HALF_KEYS})
        _REF[name] = f64, f32
    return _REF[name]


def ours(name, fp16_mode=1, qkv_dtype=torch.float16):
    from ao_amd.swin3d import crse_attention, window_map

    def fn(t, qkv, tq, tk, tv, rows, s, H):
        wmap = window_map(_dev(t["grid_coord"]), _dev(t["batch"]), SC.CASES[name][0], SC.CASES[name][1])
        return crse_attention(qkv, wmap, _dev(t["signals"])[wmap.order.long()].contiguous(), tq, tk, tv, rows, s, H, fp16_mode=fp16_mode)

    return run(name, fn, torch.float32, qkv_dtype)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_half_path_against_float64(name):
    (f64, f32), res = reference(name), ours(name)
    assert set(res) == set(f64) == set(f32) == KEYS
    bad = []
    for key in sorted(KEYS):
        assert torch.isfinite(res[key]).all(), key
        assert res[key].dtype == (torch.float16 if key in HALF_KEYS else torch.float32), key
        got, eager = _l2(res[key], f64[key]), _l2(f32[key], f64[key])
        print("swin-f16-ratio %-16s %-10s kernel %.3e  eager %.3e  ratio %.3f" % (name, key, got, eager, got / max(eager, FLOOR[key])))
        if not got <= M[key] * max(eager, FLOOR[key]):
            bad.append((key, got, M[key] * max(eager, FLOOR[key])))
    assert not bad, bad


@pytest.mark.parametrize("qkv_dtype,fp16_mode,expect", [(torch.float16, 1, torch.float16), (torch.float16, 2, torch.float16),
                                                         (torch.float16, 0, torch.float32), (torch.float32, 1, torch.float32),
                                                         (torch.float16, 3, None)],
                         ids=["half-1", "half-2", "half-0", "fp32-1", "mode-3"])
def test_routing(qkv_dtype, fp16_mode, expect):
    if expect is None:
        with pytest.raises(ValueError):
            ours("tile-edge", fp16_mode, qkv_dtype)
        return
    res = ours("tile-edge", fp16_mode, qkv_dtype)
    assert res["out"].dtype == expect and res["g_qkv"].dtype == qkv_dtype and res["g_q_table"].dtype == torch.float32
    if qkv_dtype == torch.float32:   # fp16_mode changes nothing for an fp32 qkv
        plain = ours("tile-edge", 0, qkv_dtype)
        assert all(torch.equal(res[k], plain[k]) for k in ("out", "g_qkv"))


def test_two_runs_give_the_same_bits():
    a, b = ours("dense-5"), ours("dense-5")
    assert all(torch.equal(a[k], b[k]) for k in HALF_KEYS)


def test_layer_under_autocast(monkeypatch):
    from ao_amd.swin3d import BasicLayer

    torch.manual_seed(0)
    layer = BasicLayer(48, 2, 6, 5, 4, drop_path=0.0, cRSE="XYZ_RGB_NORM", fp16_mode=1).cuda().train()
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if k.endswith("_table"):
                p.normal_(std=0.5)
    t = SC.cloud("two-clouds")
    grid, batch, local, colors = (torch.from_numpy(t[k]).cuda() for k in ("grid_coord", "batch", "local_xyz", "colors"))
    rng = np.random.default_rng(5)
    feats, g_out = (torch.from_numpy(rng.standard_normal((len(grid), 48)).astype(np.float32)).cuda() for _ in range(2))
    names = [k for k, _ in layer.named_parameters()]

    def run_layer():
        x = feats.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = layer(x, grid, batch, local, colors)
        grads = torch.autograd.grad(out, [x] + [p for _, p in layer.named_parameters()], g_out.to(out.dtype))
        return dict(zip(["out", "g_feats"] + ["g_" + k for k in names], (out.detach(),) + grads))

    res = run_layer()
    monkeypatch.setenv("AO_AMD_SWIN3D", "torch")
    ref = run_layer()
    assert set(res) == set(ref) == {"out", "g_feats"} | {"g_" + k for k in names}
    bad = []
    for key in sorted(res):
        got, m = _l2(res[key], ref[key]), M_LAYER.get(key, M_LAYER["g_param"])
        print("swin-f16-layer-ratio %-40s distance %.3e  ratio %.3f" % (key, got, got / 2.0 ** -11))
        if not got <= m * 2.0 ** -11:
            bad.append((key, got, m * 2.0 ** -11))
    assert not bad, bad
