"""GPU: every form of the sparse convolutions (ao_amd/csrc/spconv.hip through ao_amd.spunet.subm_conv / down_conv /
inverse_conv) against the restatement of tests/spunet_ref.py in float64 on the device, on both paths (HIP and
AO_AMD_SPUNET=torch).

out, g_in and g_W are compared, and the compared key set is asserted.  The bound follows tests/test_gpu_gva_f64.py and
tests/test_gpu_ptv1_layer.py: e_kernel <= M[output] * e_eager, e_eager the fp32 run of the restatement's own distance from
float64 on the same inputs and device, floored at 2^-24 (no fp32 result can be asked to lie closer to float64 than half a unit
in the last place), in relative L2 for everything and in the largest element error over the largest reference element for the
forward output.  M per output: twice the worst ratio measured on the MI355X over all cases and both paths, rounded up to a power
of two (DESIGN.md section 11 holds the table); none is above 64.

The op side takes its tables from the library (ao_amd.spunet.build_tables), the restatement from the brute-force builder:
the two agree on the order of the coarse rows (ascending (cloud, x, y, z)), so the rows compare one to one."""
import pytest
import torch

from tests import spunet_cases as SC
from tests import spunet_ref as R

pytestmark = pytest.mark.gpu

KEYS = {"out", "g_in", "g_W"}
# M per output: 2 x the worst e_kernel / e_eager over every case and both paths, as a power of two
M = {"out": 16, "g_in": 16, "g_W": 4}
FLOOR = 2.0 ** -24

_CACHE = {}


def _geometry(rows):
    """coord, offset, the brute-force tables on the device and the library's, once per row case"""
    from ao_amd import spunet

    if rows not in _CACHE:
        coord, offset = SC.lattice(SC.CONV_ROWS[rows], 20 + len(rows))
        ref = R.tables_to(R.build_tables(coord, offset, levels=2), "cuda")
        ours = spunet.build_tables(torch.from_numpy(coord).cuda(), torch.from_numpy(offset).cuda())
        _CACHE[rows] = (ref, ours, {})
    return _CACHE[rows]


def _ref_conv(case, t, x, w):
    if case.form in ("subm", "stem"):
        return R.gather(x, t["nbr5"] if case.k == 125 else t["nbr3"][0], w)
    if case.form == "down":
        return R.gather(x, t["child"][0], w)
    return R.scatter(x, t["child"][0], w, t["n"][0])


def _op_conv(case, tables, x, w):
    from ao_amd import spunet

    if case.form in ("subm", "stem"):
        return spunet.subm_conv(x, w, tables, 0, 5 if case.k == 125 else 3)
    if case.form == "down":
        return spunet.down_conv(x, w, tables, 0)
    return spunet.inverse_conv(x, w, tables, 0)


def _run(fn, inputs, dtype):
    x = inputs["x"].to(dtype).requires_grad_(True)
    w = inputs["weight"].to(dtype).requires_grad_(True)
    out = fn(x, w)
    g_in, g_w = torch.autograd.grad(out, [x, w], inputs["g_out"].to(dtype))
    return {"out": out.detach(), "g_in": g_in, "g_W": g_w}


def _reference(case, rows):
    ref, ours, cache = _geometry(rows)
    if case not in cache:
        cache.clear()
        inputs = {k: torch.from_numpy(v).cuda() for k, v in SC.conv_inputs(case, rows, ref["n"]).items()}
        fn = lambda x, w: _ref_conv(case, ref, x, w)  # noqa: E731
        cache[case] = (inputs, _run(fn, inputs, torch.float64), _run(fn, inputs, torch.float32))
    return (ours,) + cache[case]


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def _peak(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def check(res, f64, f32):
    assert set(res) == KEYS and set(f64) == KEYS and set(f32) == KEYS
    bad = []
    for key in sorted(KEYS):
        assert res[key].shape == f64[key].shape and res[key].dtype == torch.float32 and torch.isfinite(res[key]).all(), key
        kinds = [("l2", _l2(res[key], f64[key]), M[key] * max(_l2(f32[key], f64[key]), FLOOR))]
        if key == "out":
            kinds.append(("peak", _peak(res[key], f64[key]), M[key] * max(_peak(f32[key], f64[key]), FLOOR)))
        for kind, got, allowed in kinds:
            print("spunet-ratio %-5s %-4s kernel %.3e  allowed %.3e  ratio-to-eager %.3f" % (key, kind, got, allowed, got / (allowed / M[key])))
            if not got <= allowed:
                bad.append((key, kind, got, allowed))
    assert not bad, bad


def _id(case):
    return "%s-%d-%d" % (case.form, case.cin, case.cout)


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("rows", sorted(SC.CONV_ROWS))
@pytest.mark.parametrize("case", SC.CONV_SHAPES, ids=_id)
def test_conv_against_float64(case, rows, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", path)
    tables, inputs, f64, f32 = _reference(case, rows)
    print("spunet-case", _id(case), rows, path)
    check(_run(lambda x, w: _op_conv(case, tables, x, w), inputs, torch.float32), f64, f32)


@pytest.mark.parametrize("case", [SC.CONV_SHAPES[i] for i in (2, 5, 7, 9)], ids=_id)
def test_second_identical_call_is_bit_equal(case, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    tables, inputs, _, _ = _reference(case, "many")
    a, b = (_run(lambda x, w: _op_conv(case, tables, x, w), inputs, torch.float32) for _ in range(2))
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key


def test_missing_kernel_is_an_error(monkeypatch):
    from ao_amd import spunet

    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    _, tables, _ = _geometry("small")
    n = tables.n[0]
    with pytest.raises(ValueError, match="no kernel"):
        spunet.subm_conv(torch.zeros(n, 48, device="cuda"), torch.zeros(32, 3, 3, 3, 48, device="cuda"), tables, 0)
    with pytest.raises(ValueError, match="input must be"):
        spunet.subm_conv(torch.zeros(n + 1, 32, device="cuda"), torch.zeros(32, 3, 3, 3, 32, device="cuda"), tables, 0)


def test_autocast_takes_fp32(monkeypatch):
    from ao_amd import spunet

    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    case = SC.CONV_SHAPES[0]
    tables, inputs, _, _ = _reference(case, "small")
    plain = spunet.subm_conv(inputs["x"], inputs["weight"], tables, 0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = spunet.subm_conv(inputs["x"].bfloat16().float(), inputs["weight"], tables, 0)
        same = spunet.subm_conv(inputs["x"], inputs["weight"], tables, 0)
    assert cast.dtype == torch.float32 and torch.equal(same, plain)
