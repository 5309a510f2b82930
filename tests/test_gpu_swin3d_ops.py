"""GPU: ao_amd.swin3d's operators (ao_amd/csrc/swin_map.hip, swin_attention.hip) against tests/swin3d_ref.py.

Exact: the window map against a dictionary-built partition, plain and shifted, for every case of tests/swin3d_cases.py; two runs
give the same bits for out and g_qkv; a shape outside the supported set raises ValueError.

Against float64: out, g_qkv and the three table gradients of crse_attention; the compared key set is asserted.  The bound is the
rule of tests/test_gpu_octformer_ops.py: e_kernel <= M[key] * max(e_eager, 2^-24) in relative L2, e_eager the distance from
float64 of the fp32 run of swin3d_ref on the same device and inputs.  M per key: twice the worst ratio measured on the MI355X
over all cases, rounded up to a power of two."""
import numpy as np
import pytest
import torch

from tests import swin3d_cases as SC
from tests import swin3d_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
KEYS = {"out", "g_qkv", "g_q_table", "g_k_table", "g_v_table"}
# M per key: 2 x the worst e_kernel / max(e_eager, 2^-24) over every case, as a power of two
M = {"out": 4, "g_qkv": 4, "g_q_table": 4, "g_k_table": 4, "g_v_table": 4}

_REF = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


# ------------------------------------------------------------------------------------------------------- exact ----
@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "shifted"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_window_map_equals_the_dictionary(name, shifted):
    from ao_amd.swin3d import window_map

    ws = SC.CASES[name][0]
    shift = ws // 2 if shifted else 0
    t = SC.cloud(name)
    parts, slot = SC.partition(t["grid_coord"], t["batch"], ws, shift)
    wmap = window_map(_dev(t["grid_coord"]), _dev(t["batch"]), ws, shift)
    order, offsets = wmap.order.cpu().numpy(), wmap.offsets.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(len(slot))) and offsets[0] == 0 and offsets[-1] == len(slot)
    assert wmap.W == len(parts) == len(offsets) - 1 and wmap.m_max == max(len(p) for p in parts.values())
    assert np.array_equal(wmap.w_w_xyz.cpu().numpy(), slot[order])
    mine = [order[a:b].tolist() for a, b in zip(offsets[:-1], offsets[1:])]
    assert sorted(mine) == sorted(parts.values())   # the same voxels per window, w_w_id ascending inside each


def test_window_map_refuses_duplicates():
    from ao_amd.swin3d import window_map

    with pytest.raises(ValueError):
        window_map(_dev(np.array([[1, 2, 3], [4, 4, 4], [1, 2, 3]])), _dev(np.array([0, 0, 0])), 5, 0)


# ------------------------------------------------------------------------------------------ against float64 ----
def run(name, fn, dtype):
    ws, shift, H, hd, _, _, _ = SC.CASES[name]
    t = SC.attention_inputs(name)
    qkv, tq, tk, tv = (_dev(t[k]).to(dtype).requires_grad_(True) for k in ("qkv", "q_table", "k_table", "v_table"))
    out = fn(t, qkv, tq, tk, tv, SC.table_rows(name), hd ** -0.5, H)
    grads = torch.autograd.grad(out, (qkv, tq, tk, tv), _dev(t["g_out"]).to(dtype))
    return dict(zip(("out", "g_qkv", "g_q_table", "g_k_table", "g_v_table"), (out.detach(),) + grads))


def reference(name):
    if name not in _REF:
        _REF[name] = tuple(run(name, lambda t, qkv, tq, tk, tv, rows, s, H: R.attention(qkv, t["parts"], _dev(t["signals"]), tq, tk, tv, rows, s, H), dt)
                           for dt in (torch.float64, torch.float32))
    return _REF[name]


def ours(name):
    from ao_amd.swin3d import crse_attention, window_map

    def fn(t, qkv, tq, tk, tv, rows, s, H):
        wmap = window_map(_dev(t["grid_coord"]), _dev(t["batch"]), SC.CASES[name][0], SC.CASES[name][1])
        return crse_attention(qkv, wmap, _dev(t["signals"])[wmap.order.long()].contiguous(), tq, tk, tv, rows, s, H)

    return run(name, fn, torch.float32)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_crse_attention_against_float64(name):
    (f64, f32), res = reference(name), ours(name)
    assert set(res) == set(f64) == set(f32) == KEYS
    bad = []
    for key in sorted(KEYS):
        assert torch.isfinite(res[key]).all(), key
        got, eager = _l2(res[key], f64[key]), _l2(f32[key], f64[key])
        print("swin-ratio %-16s %-10s kernel %.3e  eager %.3e  ratio %.3f" % (name, key, got, eager, got / max(eager, FLOOR)))
        if not got <= M[key] * max(eager, FLOOR):
            bad.append((key, got, M[key] * max(eager, FLOOR)))
    assert not bad, bad


# ------------------------------------------------------------------------------------- repeatability, limits ----
def test_two_runs_give_the_same_bits():
    a, b = ours("dense-5"), ours("dense-5")
    assert all(torch.equal(a[k], b[k]) for k in ("out", "g_qkv"))


@pytest.mark.parametrize("H,hd,ws,rows", [(6, 12, 5, (20,)), (65, 8, 5, (20,)), (6, 16, 8, (32,)), (6, 16, 5, (21,))],
                         ids=["hd-12", "heads-65", "window-8", "table-rows"])
def test_outside_the_supported_shapes_raises(H, hd, ws, rows):
    from ao_amd.swin3d import crse_attention, window_map

    grid, batch = torch.arange(30, device="cuda").view(10, 3), torch.zeros(10, dtype=torch.long, device="cuda")
    table = torch.zeros(6 * 20 * H * hd, device="cuda")
    with pytest.raises(ValueError):
        wmap = window_map(grid, batch, ws, 0)
        crse_attention(torch.zeros(10, 3 * H * hd, device="cuda"), wmap, torch.zeros(10, 3, device="cuda"), table, table, table, rows, 0.25, H)
