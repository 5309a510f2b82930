"""GPU: the bf16-operand forms of the sparse convolutions (ao_amd/csrc/spconv_bf16.hip through operands="bf16" of
ao_amd.spunet.subm_conv / down_conv / inverse_conv) and SpUNetBase(conv_operands="bf16") against tests/spunet_ref.py in float64.

Exact: x and g_out integers in [-4, 4], weights from {-1, -1/2, 0, 1/2, 1}: every operand is a bf16 value and every partial sum
a multiple of 1/2 below 2^24 (27 * 384 * 4 = 41 472; 3001 * 16 = 48 016), so fp32 accumulation in any order is exact and out,
g_in, g_W must EQUAL the float64 restatement.  A wrong lane, pitch, transpose or skipped wave cannot pass.
Rounded random: SC.conv_inputs against the float64 restatement on x, weight, g_out rounded through .bfloat16(): the kernel's only
error is then its fp32 accumulation, so the bound is the M-rule of tests/test_gpu_spunet_conv.py, e_kernel <= M max(e_eager,
2^-24), e_eager the fp32 restatement on the same rounded operands.  The op takes the unrounded x and weight on both paths; the
eager path rounds no gradient, so it alone is handed the rounded g_out.
Model: the HIP run's relative-L2 distance from the UNROUNDED float64 restatement is at most M times the AO_AMD_SPUNET=torch bf16
run's (both are bf16 rounding noise; the two round different fp32 intermediates and cannot be compared to each other).
M: twice the worst ratio measured on the MI355X, rounded up to a power of two, at least 1, at most 64 (DESIGN.md section 18,
profiles/spunet_bf16_ratios.txt).  Every ratio is printed as a `spunet-bf16-ratio` line."""
import pytest
import torch

from tests import spunet_cases as SC
from tests import spunet_ref as R

pytestmark = pytest.mark.gpu

CASES = tuple(c for c in SC.CONV_SHAPES if c.form != "stem")
MANY = tuple(c for c in CASES if (c.form, c.cin, c.cout) in (("subm", 128, 96), ("inverse", 128, 96)))
PAIRS = [(c, rows) for c in CASES for rows in ("small", "ragged")] + [(c, "many") for c in MANY]
IDS = ["%s-%d-%d-%s" % (c.form, c.cin, c.cout, rows) for c, rows in PAIRS]
# worst ratios measured: out 2.29 / 3.83 (L2 / largest element), g_in 2.42, g_W 1.00; model logits 1.006, gradients 1.47
M = {"out": 8, "g_in": 8, "g_W": 2}
M_MODEL = {"logits": 4, "grad": 4}
FLOOR = 2.0 ** -24
_GEO, _REF = {}, {}


def _geometry(rows):
    from ao_amd import spunet

    if rows not in _GEO:
        coord, offset = SC.lattice(SC.CONV_ROWS[rows], 20 + len(rows))
        _GEO[rows] = (R.tables_to(R.build_tables(coord, offset, levels=2), "cuda"),
                      spunet.build_tables(torch.from_numpy(coord).cuda(), torch.from_numpy(offset).cuda()))
    return _GEO[rows]


def _ref_conv(case, t, x, w):
    if case.form == "inverse":
        return R.scatter(x, t["child"][0], w, t["n"][0])
    return R.gather(x, t["child"][0] if case.form == "down" else t["nbr3"][0], w)


def _op_conv(case, tables, x, w, operands="bf16"):
    from ao_amd import spunet

    fn = {"subm": spunet.subm_conv, "down": spunet.down_conv, "inverse": spunet.inverse_conv}[case.form]
    return fn(x, w, tables, 0, operands=operands)


def _run(fn, inputs, dtype):
    x = inputs["x"].to(dtype).requires_grad_(True)
    w = inputs["weight"].to(dtype).requires_grad_(True)
    out = fn(x, w)
    g_in, g_w = torch.autograd.grad(out, [x, w], inputs["g_out"].to(dtype))
    return {"out": out.detach(), "g_in": g_in, "g_W": g_w}


def _random(case, rows):
    return {k: torch.from_numpy(v).cuda() for k, v in SC.conv_inputs(case, rows, _geometry(rows)[0]["n"]).items()}


@pytest.mark.parametrize("case,rows", PAIRS, ids=IDS)
def test_exact_on_bf16_valued_inputs(case, rows, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    ref, ours = _geometry(rows)
    gen = torch.Generator().manual_seed(7)
    inputs = {k: v.shape for k, v in SC.conv_inputs(case, rows, ref["n"]).items()}
    inputs = {k: (torch.randint(-2, 3, s, generator=gen) * 0.5 if k == "weight" else torch.randint(-4, 5, s, generator=gen)).float().cuda()
              for k, s in inputs.items()}
    want = _run(lambda x, w: _ref_conv(case, ref, x, w), inputs, torch.float64)
    got = _run(lambda x, w: _op_conv(case, ours, x, w), inputs, torch.float32)
    for key in ("out", "g_in", "g_W"):
        assert got[key].dtype == torch.float32 and torch.equal(got[key], want[key].float()), key


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def _peak(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("case,rows", PAIRS, ids=IDS)
@pytest.mark.parametrize("path", ["hip", "torch"])
def test_rounded_random_against_float64(case, rows, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", path)
    ref, ours = _geometry(rows)
    if (case, rows) not in _REF:  # (once for both paths)
        raw = _random(case, rows)
        rounded = {k: v.bfloat16().float() for k, v in raw.items()}
        fn = lambda x, w: _ref_conv(case, ref, x, w)  # noqa: E731
        _REF.clear()
        _REF[case, rows] = (raw, rounded, _run(fn, rounded, torch.float64), _run(fn, rounded, torch.float32))
    raw, rounded, f64, f32 = _REF[case, rows]
    got = _run(lambda x, w: _op_conv(case, ours, x, w), dict(raw, g_out=rounded["g_out"]) if path == "torch" else raw, torch.float32)
    bad = []
    for key in ("out", "g_in", "g_W"):
        assert got[key].dtype == torch.float32 and torch.isfinite(got[key]).all(), key
        for kind, dist in (("l2", _l2),) + ((("peak", _peak),) if key == "out" else ()):
            e, eager = dist(got[key], f64[key]), max(dist(f32[key], f64[key]), FLOOR)
            print("spunet-bf16-ratio %-28s %-5s %-4s %-5s kernel %.3e eager %.3e ratio %.3f" % (IDS[PAIRS.index((case, rows))], path, key, kind, e, eager, e / eager))
            if not e <= M[key] * eager:
                bad.append((key, kind, e, eager))
    assert not bad, bad


@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[8]], ids=["subm", "down", "inverse"])
def test_second_identical_call_is_bit_equal(case, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    ours, inputs = _geometry("many")[1], _random(case, "many")
    a, b = (_run(lambda x, w: _op_conv(case, ours, x, w), inputs, torch.float32) for _ in range(2))
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_operands_keyword(monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    case = CASES[0]
    ours, inputs = _geometry("small")[1], _random(case, "small")
    run = lambda operands: _op_conv(case, ours, inputs["x"], inputs["weight"], operands)  # noqa: E731
    fp32, bf16 = run("fp32"), run("bf16")
    assert not torch.equal(fp32, bf16) and torch.equal(run("autocast"), fp32)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = run("autocast")
        assert torch.equal(run("fp32"), fp32)
    assert cast.dtype == torch.float32 and torch.equal(cast, bf16)
    with pytest.raises(ValueError, match="operands"):
        run("fp16")


def _step(model, batch, dtype=torch.float32, tables=None):
    model.load_state_dict(SC.fill_state(SC.shapes_of(R.SpUNet(6, 13)), SC.MODEL_SEED), strict=True)
    model = model.to(device="cuda", dtype=dtype).train()
    batch = dict(batch, feat=batch["feat"].to(dtype))
    logits = model(batch) if tables is None else model(batch, tables)
    torch.nn.functional.cross_entropy(logits, batch["segment"]).backward()
    res = {"logits": logits.detach()}
    res.update({"g:" + k: p.grad for k, p in model.named_parameters()})
    return res


def test_model_step_with_bf16_operands(monkeypatch):
    from ao_amd import spunet

    batch = {k: torch.from_numpy(v).cuda() for k, v in SC.model_batch().items()}
    tables = R.tables_to(R.build_tables(batch["discrete_coord"].cpu().numpy(), batch["offset"].cpu().numpy()), "cuda")
    f64 = _step(R.SpUNet(6, 13), batch, torch.float64, tables)
    runs = {}
    for path in ("hip", "torch"):
        monkeypatch.setenv("AO_AMD_SPUNET", path)
        runs[path] = _step(spunet.SpUNetBase(6, 13, conv_operands="bf16"), batch)
    assert set(spunet.SpUNetBase(6, 13, conv_operands="bf16").state_dict()) == set(spunet.SpUNetBase(6, 13).state_dict())
    assert set(runs["hip"]) == set(f64) and len(f64) == 1 + len(list(R.SpUNet(6, 13).parameters()))
    bad = []
    for key in sorted(f64):
        assert torch.isfinite(runs["hip"][key]).all(), key
        e, eager = _l2(runs["hip"][key], f64[key]), _l2(runs["torch"][key], f64[key])
        print("spunet-bf16-ratio model %-44s hip %.3e torch %.3e ratio %.3f" % (key, e, eager, e / eager))
        if not e <= M_MODEL["logits" if key == "logits" else "grad"] * eager:
            bad.append((key, e, eager))
    assert not bad, bad
