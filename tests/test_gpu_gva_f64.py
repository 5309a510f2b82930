"""GPU: every form of the grouped-vector-attention kernels (ao_amd/csrc/gva_*.hip) against a float64 reference.

Reference: tests/gva_ref64.py -- tests/gva_torch_ref.py::TorchImpl (+ the grouped projection) on float64 copies of the inputs,
every gradient from float64 autograd, on inputs whose ReLU pre-activations are exact in fp32 (no mask bit can differ, exact
zeros planted at both kinks; asserted per case).  The bound is relative to the eager fp32 statement's OWN distance from float64
on the same inputs and device:

    e_kernel = |kernel - f64| / |f64|   <=   M[output] * e_eager,    e_eager = |TorchImpl_fp32 - f64| / |f64|

in relative L2 and in the largest element error over the largest reference element.  M is per output, twice the worst ratio
measured on the MI355X rounded up to a power of two (DESIGN.md 3.4 "parity against float64" holds the table); the kernels use
the hardware exp2 / reciprocal, fp32 matrix instructions with another summation order and fixed-order partial records, which the
eager statement does not.  Outputs whose true value is 0 (gbw2) are bounded by M x the eager statement's own absolute noise.

Forms (whichever exist for the shape; no case and no output is left out -- the compared keys are asserted against the list):
  point     _HipImpl.logits / aggregate / project through autograd (the matrix-core point kernels where they are the default)
  flat      the same with AO_AMD_BWD_STAGED=1 (one lane per slot)
  staged    gva_aggregate_forward + gva_peb_forward, gva_peb_backward + gva_aggregate_backward launchers
  tile      gva_attention_forward (A requested) + gva_attention_backward + gva_attention_wgrad launchers
  tile_noA  gva_attention_forward without A"""
import os

import pytest
import torch

from tests import gva_ref64 as R

pytestmark = pytest.mark.gpu

# M per output: 2 x the worst e_kernel / e_eager over every case and form, rounded up to a power of two
M = dict(W1=8, T1=32, T2=16, w=4, sw=4, A=4, out_v=8, out=8,
         gkW=16, gqW=8, lga=8, lgb=8, gM=8, gcW=16,
         gW1=32, gsc=8, gsh=16, gWw2=16, gbw2=64, gv=4, ga=4, gb=4, gWp2=8, gbp2=8)

BWD8 = ("gW1", "gsc", "gsh", "gWw2", "gbw2", "gv", "ga", "gb")


def forms_of(case):
    tile = case.k == 16 and (case.c, case.g) in R.TILE_SHAPES
    return ("point", "flat", "staged") + (("tile", "tile_noA") if tile else ())


def expected_keys(case, form):
    bwd = case.kind != "spread"
    if form in ("point", "flat"):
        return set(R.FWD_LOGITS + ("sw", "A", "out_v", "out")) | (set(R.BWD_LOGITS + R.BWD_ATTN) if bwd else set())
    if form == "staged":
        return set(R.FWD_ATTN) | (set(BWD8) if bwd else set())
    if form == "tile_noA":
        return {"w", "sw", "out"}
    keys = {"w", "sw", "A", "out"}
    if bwd:
        keys |= {"gWp2", "gbp2"}
        if (case.c, case.g) in R.BWD_TILE_SHAPES:
            keys |= set(BWD8)
    return keys


PAIRS = [pytest.param(case, form, id="%s-%s" % (case.name, form)) for case in R.CASES for form in forms_of(case)]


def _gpu_knn(k, coord, offset):
    from ao_amd import pointops

    return pointops.knn_query(k, coord, offset)[0]


_CACHE = {}


def reference(case):
    """(inputs, float64 reference, eager fp32 statement) of a case, computed once (the forms of a case run back to back)"""
    if case.name not in _CACHE:
        _CACHE.clear()
        t = R.build_inputs(case, _gpu_knn, device="cuda")
        R.check_inputs(case, t)
        bwd = case.kind != "spread"
        _CACHE[case.name] = (t, R.statement(t, torch.float64, bwd), R.statement(t, torch.float32, bwd))
    return _CACHE[case.name]


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _run_autograd(t, bwd):
    from ao_amd.ptv2.gva import _HipImpl

    leaf = lambda key: t[key].clone().requires_grad_(bwd)
    coord, idx = t["coord"], t["idx"]
    L = [leaf(key) for key in ("kW", "qW", "a", "b", "M", "cW")]
    W1, T1, T2 = _HipImpl.logits(*L, coord, idx)
    S = [leaf(key) for key in ("W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b")]
    Wp2, bp2 = leaf("Wp2"), leaf("bp2")
    out_v, A, sw = _HipImpl.aggregate(*S, coord, idx)
    out = _HipImpl.project(A, Wp2, bp2, sw, out_v)
    res = dict(W1=W1, T1=T1, T2=T2, sw=sw, A=A, out_v=out_v, out=out)
    if bwd:
        res.update(zip(R.BWD_LOGITS, torch.autograd.grad([W1, T1, T2], L, [t["g_W1"], t["g_T1"], t["g_T2"]])))
        res.update(zip(R.BWD_ATTN, torch.autograd.grad(out, S + [Wp2, bp2], t["g_out"])))
    return {key: val.detach() for key, val in res.items()}


def _p(t, *keys):
    return [t[key].data_ptr() for key in keys]


def _bwd_buffers(n, k, c, g):
    return dict(gW1=_nan(n, k, g), gsc=_nan(g), gsh=_nan(g), gWw2=_nan(g, g), gbw2=_nan(g), gv=_nan(n, c), ga=_nan(c, 3), gb=_nan(c))


def _run_staged(t, n, k, c, g, bwd):
    from ao_amd import _lib
    from ao_amd.ptv2.gva import inverse_table

    L, st = _lib.lib(), _lib.stream_ptr()
    o = dict(out_v=_nan(n, c), A=_nan(n, g, c), sw=_nan(n, g), w=_nan(n, k, g), out=_nan(n, c))
    _lib.check(L.gva_aggregate_forward_hip_launcher(
        n, k, c, g, *_p(t, "W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b", "coord", "idx"), *_p(o, "out_v", "A", "sw", "w"), st),
        "gva_aggregate_forward_hip_launcher")
    _lib.check(L.gva_peb_forward_hip_launcher(n, c, g, o["A"].data_ptr(), *_p(t, "Wp2", "bp2"), *_p(o, "sw", "out_v", "out"), st),
               "gva_peb_forward_hip_launcher")
    if bwd:
        inv_ptr, inv_rows = inverse_table(t["idx"])
        gA, g_sw = _nan(n, g, c), _nan(n, g)
        _lib.check(L.gva_peb_backward_hip_launcher(n, c, g, *_p(t, "g_out", "Wp2", "bp2"), gA.data_ptr(), g_sw.data_ptr(), st),
                   "gva_peb_backward_hip_launcher")
        b = _bwd_buffers(n, k, c, g)
        ws = _lib.workspace(L.gva_aggregate_workspace_bytes(n, k, c, g), t["v"].device)
        _lib.check(L.gva_aggregate_backward_hip_launcher(
            n, k, c, g, *_p(t, "W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b", "coord", "idx"), o["w"].data_ptr(), t["g_out"].data_ptr(),
            gA.data_ptr(), g_sw.data_ptr(), inv_ptr.data_ptr(), inv_rows.data_ptr(), *_p(b, *BWD8), ws.data_ptr(), ws.numel(), st),
            "gva_aggregate_backward_hip_launcher")
        o.update(b)
    torch.cuda.synchronize()
    return o


def _run_tile(t, n, k, c, g, bwd, want_a):
    from ao_amd import _lib
    from ao_amd.ptv2.gva import inverse_table

    L, st = _lib.lib(), _lib.stream_ptr()
    o = dict(w=_nan(n, k, g), sw=_nan(n, g), out=_nan(n, c))
    if want_a:
        o["A"] = _nan(n, g, c)
    _lib.check(L.gva_attention_forward_hip_launcher(
        n, k, c, g, *_p(t, "W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b", "coord", "idx", "Wp2", "bp2"), *_p(o, "w", "sw", "out"),
        o["A"].data_ptr() if want_a else 0, st), "gva_attention_forward_hip_launcher")
    if bwd and want_a:
        dev = t["v"].device
        if (c, g) in R.BWD_TILE_SHAPES:
            inv_ptr, inv_rows = inverse_table(t["idx"])
            b = _bwd_buffers(n, k, c, g)
            ws = _lib.workspace(L.gva_aggregate_workspace_bytes(n, k, c, g), dev)
            _lib.check(L.gva_attention_backward_hip_launcher(
                n, k, c, g, *_p(t, "W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b", "coord", "idx"), o["w"].data_ptr(),
                *_p(t, "g_out", "Wp2", "bp2"), inv_ptr.data_ptr(), inv_rows.data_ptr(), *_p(b, *BWD8), ws.data_ptr(), ws.numel(), st),
                "gva_attention_backward_hip_launcher")
            o.update(b)
        o.update(gWp2=_nan(c, c), gbp2=_nan(c))
        ws = _lib.workspace(L.dense_workspace_bytes(n, c, c), dev)
        _lib.check(L.gva_attention_wgrad_hip_launcher(
            n, k, c, g, t["g_out"].data_ptr(), o["w"].data_ptr(), o["sw"].data_ptr(), *_p(t, "a", "b", "coord", "idx"),
            o["gWp2"].data_ptr(), o["gbp2"].data_ptr(), ws.data_ptr(), ws.numel(), st), "gva_attention_wgrad_hip_launcher")
    torch.cuda.synchronize()
    return o


def run_form(case, form, t):
    """the outputs of one kernel form on the inputs t: dict key -> tensor"""
    n, c, g, k = case.n, case.c, case.g, case.k
    bwd = case.kind != "spread"
    if form in ("point", "flat"):
        old = os.environ.pop("AO_AMD_BWD_STAGED", None)
        try:
            if form == "flat":
                os.environ["AO_AMD_BWD_STAGED"] = "1"  # (read at every call: tests/test_gpu_gva_stages.py::kernel_family)
            return _run_autograd(t, bwd)
        finally:
            os.environ.pop("AO_AMD_BWD_STAGED", None)
            if old is not None:
                os.environ["AO_AMD_BWD_STAGED"] = old
    if form == "staged":
        return _run_staged(t, n, k, c, g, bwd)
    return _run_tile(t, n, k, c, g, bwd, form == "tile")


def figures(case, form):
    """[(key, e_kernel, e_eager, m_kernel, m_eager, finite)]: relative L2 and largest-element errors against float64 of the
    kernel form and of the eager fp32 statement; for the true-zero outputs e_* = m_* = the largest absolute value"""
    t, ref, eager = reference(case)
    got = run_form(case, form, t)
    assert set(got) == expected_keys(case, form), (sorted(got), sorted(expected_keys(case, form)))
    rows = []
    for key in sorted(got):
        assert got[key].shape == ref[key].shape, (key, got[key].shape, ref[key].shape)
        finite = bool(torch.isfinite(got[key]).all())
        if key in R.ZERO_KEYS:
            ek = mk = float(got[key].double().abs().max())
            ee = me = float(eager[key].double().abs().max())
        else:
            ek, mk = R.errors(got[key], ref[key])
            ee, me = R.errors(eager[key], ref[key])
        rows.append((key, ek, ee, mk, me, finite))
    return rows


def test_the_forms_cover_every_output():
    for c, g in R.BWD_TILE_SHAPES:
        case = next(x for x in R.CASES if (x.c, x.g, x.kind) == (c, g, "std"))
        assert set().union(*(expected_keys(case, f) for f in forms_of(case))) == set(R.ALL_KEYS)
        assert set().union(*(expected_keys(case, f) for f in ("tile",))) >= {"gWp2", "gbp2", "w", "A"} | set(BWD8)
    assert set(M) == set(R.ALL_KEYS)


@pytest.mark.parametrize("case,form", PAIRS)
def test_kernel_form_against_float64(case, form):
    rows = figures(case, form)
    for key, ek, ee, mk, me, finite in rows:
        print("f64 %s %s %s e_kernel %.3e e_eager %.3e ratio %.2f | max %.3e %.3e ratio %.2f" % (
            case.name, form, key, ek, ee, ek / max(ee, 1e-300), mk, me, mk / max(me, 1e-300)))
    for key, ek, ee, mk, me, finite in rows:
        assert finite, (key, "not finite (an unwritten row shows as NaN)")
        assert ek <= M[key] * ee, (key, "relative L2", ek, ee, ek / max(ee, 1e-300), M[key])
        assert mk <= M[key] * me, (key, "largest element", mk, me, mk / max(me, 1e-300), M[key])


def test_wgrad_launcher_rejects_other_shapes():
    from ao_amd import _lib
    import ao_amd.ptv2.gva  # noqa: F401

    L = _lib.lib()
    assert L.gva_attention_wgrad_hip_launcher(64, 16, 48, 6, *([1] * 10), 1 << 20, 0) == 1    # PTV2_ERR_ARG: no instance
    assert L.gva_attention_wgrad_hip_launcher(64, 8, 96, 12, *([1] * 10), 1 << 20, 0) == 1    # k != 16
    assert L.gva_attention_wgrad_hip_launcher(0, 16, 96, 12, *([1] * 10), 0, 0) == 0          # n = 0: nothing to do
    assert L.gva_attention_wgrad_hip_launcher(64, 16, 96, 12, *([1] * 10), 16, 0) == 2        # PTV2_ERR_WORKSPACE


def test_deferred_recompute_weight_gradient_has_the_same_bits():
    """wgrad.hip::gva_wp2_wgrad_recompute claims "the same split as a filed job: the same bits either way".  The benchmark's
    scene (levels of 18 905 x 96, 4 501 x 192, 1 074 x 384 points): grad of every deep level's attn.linear_p_bias.3 with the
    weight gradients filed and run batched at the end of the backward (wp2_wgrad_tile_kernel_jobs behind the posrel pre-pass;
    the default) against every launch where it is called (AO_AMD_WGRAD_DEFER=0, here through the same switch's setter
    ptv2_wgrad_defer_mode, as tests/test_gpu_native_model.py does), bit for bit."""
    import torch.nn.functional as F

    import ao_amd.ptv2 as ptv2
    from ao_amd import _lib, synth
    from ao_amd.ptv2.parallel import scene_seeds
    from oracle import ptv2_ref

    L = _lib.lib()
    cfg = dict(ptv2_ref.S3DIS_CFG, drop_path_rate=0.0)
    b = synth.scene_batch(scene_seeds(0, 1), point_max=120000, in_channels=cfg["in_channels"], num_classes=cfg["num_classes"], room=1)
    data = {key: torch.from_numpy(val).cuda() for key, val in b.items()}
    prev = L.ptv2_wgrad_defer_mode(-1)
    res = {}
    try:
        for mode in (1, 0):
            L.ptv2_wgrad_defer_mode(mode)
            model = ptv2.PointTransformerV2(**cfg).cuda()
            model.load_state_dict(ptv2_ref.init_state(cfg, seed=31), strict=True)
            model.train()
            loss = F.cross_entropy(model(data).float(), data["segment"], ignore_index=-1)
            loss.backward()
            res[mode] = {name: p.grad.detach().clone() for name, p in model.named_parameters() if "attn.linear_p_bias.3." in name}
    finally:
        L.ptv2_wgrad_defer_mode(prev)
    deep = [name for name, gr in res[1].items() if gr.shape[0] in (96, 192, 384, 512)]
    assert {res[1][name].shape[0] for name in deep} >= {96, 192, 384} and len(deep) >= 12
    for name in deep:
        assert bool(torch.isfinite(res[1][name]).all()) and float(res[1][name].abs().max()) > 0
        assert torch.equal(res[1][name], res[0][name]), (name, float((res[1][name] - res[0][name]).abs().max()))
