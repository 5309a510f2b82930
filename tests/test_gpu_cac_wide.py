"""GPU: the CAC launchers at 64 < C <= 128 (ao_amd/csrc/cac_mfma.hip: the K x C and rows x K products on the fp32 matrix
instruction) against the float64 statements of tests/cac_ref64.py, to the derived bounds of `cac_ref64.compare`.

Cases, inputs, variants and runners are those of tests/cac_cases.py and tests/test_gpu_cac_f64.py; only the shapes are new, the
smallest that reach each edge of the wide kernels (C % 16 = 4, K one past a 16-tile and one past a class group, a row past a
stage of 64 and past a chunk, an empty scene, ten slabs, every limit at once)."""
import numpy as np
import pytest
import torch

from tests import cac_cases as C
from tests import cac_ref64 as R
from tests import test_gpu_cac_f64 as T

pytestmark = pytest.mark.gpu

# (K, C, rows per scene, thr)
GRID = ((1, 68, (1,), 0.0), (17, 96, (65,), 0.0), (20, 96, (257,), 0.0), (20, 96, (300, 0, 17), 0.75),
        (65, 68, (1000, 990, 1010), 0.0), (200, 96, (17,), 0.75), (200, 96, (2305,), 0.0), (256, 128, (257,), 0.75))
CASES = {(k, c, sizes): C.Case("k%d-c%d-%s-thr%g" % (k, c, "_".join(map(str, sizes)), thr), "scene", dict(k=k, c=c, sizes=sizes, thr=thr), ())
         for k, c, sizes, thr in GRID}
PAIRS = [pytest.param(case, tier, id="%s-%s" % (case.name, tier)) for case in CASES.values() for tier in C.TIERS]
LAUNCHERS = (T.WSF, T.WSB, T.COF, T.COB)

_time_limit = T._time_limit
spy = T.spy


@pytest.mark.parametrize("case,tier", PAIRS)
@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_launcher_against_float64(launcher, case, tier):
    T.check(launcher, case, tier)


@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_a_second_identical_call_gives_the_same_bits(launcher):
    case = CASES[200, 96, (2305,)]
    for var in C.variants(case, launcher):
        a, b = T.run(launcher, case, "plain", **var), T.run(launcher, case, "plain", **var)
        assert set(a) == set(b)
        for key in a:
            assert R.bits_equal(a[key], b[key]), (launcher, var, key)


@pytest.mark.parametrize("key", [(20, 96, (300, 0, 17)), (200, 96, (17,))])
@pytest.mark.parametrize("tier", C.TIERS)
def test_weighted_sum_and_cosine_through_autograd(key, tier, spy):
    from ao_amd.ptv2.cac import _Cosine, _WeightedSum

    case = CASES[key]
    t, name = C.inputs(case, tier), case.name
    off, k, rows = T._cuda(t["offset"]), t["k"], t["max_rows"]
    dout = T._cuda(t["dout_sets"])
    x, logits = T._cuda(t["x"], True), T._cuda(t["logits"], True)
    z, out = _WeightedSum.apply(x, logits, None, off, k, rows, t["thr"], C.PROTO_EPS, 0)
    T._api((T.WSF, name, tier), dict(z=z, out=out), C.reference(case, tier, T.WSF, mode=0))
    T._api((T.WSB, name, tier), dict(zip(("gx", "glogits"), torch.autograd.grad(out, (x, logits), dout))),
           C.reference(case, tier, T.WSB, mode=0))
    x = T._cuda(t["x"], True)
    z, out = _WeightedSum.apply(x, None, T._cuda(t["label"]), off, k, rows, 0.0, C.MEAN_EPS, 1)
    T._api((T.WSF, name, tier, "mode1"), dict(z=z, out=out), C.reference(case, tier, T.WSF, mode=1))
    T._api((T.WSB, name, tier, "mode1"), dict(gx=torch.autograd.grad(out, x, dout[:1])[0]), C.reference(case, tier, T.WSB, mode=1))
    for per_scene in (1, 0):
        v = C.view(case, tier, T.COF, per_scene=per_scene)
        x, q = T._cuda(t["x"], True), T._cuda(v["q"], True)
        out = _Cosine.apply(x, q, off, rows, C.COS_SCALE)
        T._api((T.COF, name, tier, "p%d" % per_scene), dict(out=out), C.reference(case, tier, T.COF, per_scene=per_scene))
        gx, gq = torch.autograd.grad(out, (x, q), T._cuda(v["dout"]))
        T._api((T.COB, name, tier, "p%d" % per_scene), dict(gx=gx, gq=gq), C.reference(case, tier, T.COB, per_scene=per_scene))
    assert set(LAUNCHERS) <= set(spy.names), spy.names


def test_limits():
    """native at C = 96 and 128, not at 132 (too wide) or 70 (C % 4); a launcher call at C = 132 is refused and writes nothing"""
    from ao_amd.ptv2.cac import native_ok

    assert [native_ok(torch.empty((8, c), device="cuda"), 20) for c in (96, 128, 132, 70)] == [True, True, False, False]
    B = T.Buffers()
    n, k, c = 40, 20, 132
    x, logits, off = B.f(np.ones((n, c))), B.f(np.ones((n, k))), B.i([n])
    big, ws = B.out((k * c + n * c,)), B.ws(1 << 20)
    assert T._bytes("cac_workspace_bytes", 1, n, n, k, c) == 0
    T._call(T.WSF, 0, n, 1, n, k, c, T._p(x), T._p(logits), 0, T._p(off), 0.0, 1e-7, T._p(big), T._p(big), T._p(ws), 1 << 20, T._st(),
            expect=T.ERR_ARG)
    T._call(T.WSB, 0, n, 1, n, k, c, T._p(x), T._p(logits), 0, T._p(off), 0.0, 1e-7, T._p(big), T._p(big), T._p(big), T._p(big), 0,
            T._st(), expect=T.ERR_ARG)
    T._call(T.COF, n, 1, n, k, c, T._p(x), T._p(big), 1, T._p(off), 15.0, T._p(big), T._st(), expect=T.ERR_ARG)
    T._call(T.COB, n, 1, n, k, c, T._p(x), T._p(big), 1, T._p(off), 15.0, T._p(big), T._p(big), T._p(big), T._p(ws), 1 << 20, T._st(),
            expect=T.ERR_ARG)
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all())
    B.intact("limits")
