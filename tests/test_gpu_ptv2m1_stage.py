"""GPU: the multiplier logits stage of PT-v2m1 (ao_amd/csrc/gva_mul.hip) against a float64 reference.

Reference: tests/ptv2m1_ref.py::logits_mul on float64 copies of the inputs, every gradient from float64 autograd, on the
inputs of tests/ptv2m1_cases.py (both ReLU pre-activations exact in fp32: no mask bit can differ; asserted per case).  The bound
is the project's M-rule, relative to the eager fp32 statement's OWN distance from float64 on the same inputs
and device, floored at 2^-24 of the reference:

    e_kernel = |kernel - f64| / |f64|   <=   M[output] * max(e_eager, 2^-24),    e_eager = |logits_mul_fp32 - f64| / |f64|

in relative L2 and in the largest element error over the largest reference element.  M is per output, twice the worst ratio
measured on the MI355X rounded up to a power of two, at most 64 (profiles/ptv2m1_ratios.txt).  Every run
prints its ratios as `ptv2m1-ratio` lines.  Two calls on the same input must return the same bits in every output.

Memory: the peak of the stage's forward + backward grows by less than ONE (N, K, C) fp32 tensor between n = 2 048 and 8 192."""
import pytest
import torch

from tests import gva_ref64 as R
from tests import ptv2m1_cases as C
from tests import ptv2m1_ref as F

pytestmark = pytest.mark.gpu

# M per output: 2 x the worst e_kernel / e_eager over every case, rounded up to a power of two, capped at 64
# (worst ratios measured: W1 1.75, T1 1.34, T2 1.25, g_key 1.84, g_query 1.78, g_w 2.11, g_a_m 1.68, g_b_m 1.89, g_Wm2 1.87,
# g_bm2 2.13, g_a 1.73, g_b 3.20, g_M 2.02, g_cW 3.24)
M = dict(W1=4, T1=4, T2=4, g_key=4, g_query=4, g_w=8, g_a_m=4, g_b_m=4, g_Wm2=4, g_bm2=8, g_a=4, g_b=8, g_M=8, g_cW=8)
FLOOR = 2.0 ** -24


def _gpu_knn(k, coord, offset):
    from ao_amd import pointops

    return pointops.knn_query(k, coord, offset)[0]


def _run(t, bwd=True):
    from ao_amd.ptv2.gva import _HipImpl

    leaves = [t[key].clone().requires_grad_(bwd) for key in F.INPUTS]
    W1, T1, T2 = _HipImpl.logits_mul(*leaves, t["coord"], t["idx"])
    res = dict(W1=W1, T1=T1, T2=T2)
    if bwd:
        res.update(zip(F.BWD, torch.autograd.grad([W1, T1, T2], leaves, [t["g_W1"], t["g_T1"], t["g_T2"]])))
    return {key: val.detach() for key, val in res.items()}


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_stage_against_float64(case):
    t = C.build_inputs(case, _gpu_knn, device="cuda")
    C.check_inputs(case, t)
    ref, eager = F.statement(t, torch.float64), F.statement(t, torch.float32)
    got, again = _run(t), _run(t)
    assert set(got) == set(F.ALL_KEYS) == set(M)
    bad = []
    for key in F.ALL_KEYS:
        assert got[key].shape == ref[key].shape and bool(torch.isfinite(got[key]).all()), key
        assert torch.equal(got[key], again[key]), (case.name, key, "two calls differ")
        ek, ee = R.errors(got[key], ref[key]), R.errors(eager[key], ref[key])
        ratios = [ek[i] / max(ee[i], FLOOR) for i in range(2)]
        print("ptv2m1-ratio %-28s %-8s l2 %8.3f max %8.3f   e_kernel %.3e %.3e  e_eager %.3e %.3e"
              % (case.name, key, ratios[0], ratios[1], ek[0], ek[1], ee[0], ee[1]))
        if not all(ek[i] <= M[key] * max(ee[i], FLOOR) for i in range(2)):
            bad.append((key, ratios))
    assert not bad, (case.name, bad)


def _peak(c, g, k, n):
    case = R.Case("mem-n%d-c%d" % (n, c), n, c, g, k, "std")
    t = C.build_inputs(case, _gpu_knn, device="cuda")
    torch.cuda.synchronize()  # (the inverse table is built inside the measured region: it belongs to the stage's footprint)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _run(t)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("c,g,k", [(48, 6, 16), (192, 24, 16)])
def test_no_buffer_grows_with_n_k_c(c, g, k):
    from ao_amd import _lib

    n0, n1 = 2048, 8192
    _peak(c, g, k, n1)  # (warm: kernels loaded, the cached workspace at its final size)
    _lib._WS.clear()
    p0 = _peak(c, g, k, n0)
    _lib._WS.clear()
    p1 = _peak(c, g, k, n1)
    one_tensor = (n1 - n0) * k * c * 4
    # what does grow with n: W1 and the (n,k,g) row gradient of the workspace (k c / 8 floats per point each, the workspace
    # allocated with a quarter to spare), the leaf copies of key / query and their gradients (4 c), the inverse table (k + 1):
    # by count (2.25 k c / 8 + 4 c + k) * 4 = 1 700 of the k c * 4 = 3 072 bytes per point at (48, 16); measured 54 % and 56 %
    print("ptv2m1-memory c %d g %d k %d: peak %d -> %d bytes, growth %d, one (N,K,C) tensor %d" % (c, g, k, p0, p1, p1 - p0, one_tensor))
    assert p1 - p0 < one_tensor, (p0, p1, one_tensor)
