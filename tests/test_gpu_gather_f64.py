"""GPU: the 14 launchers of ao_amd/csrc/gather_ops.hip and the 4 of ao_amd/csrc/pool.hip against float64.

Reference: tests/gather_ref64.py -- float64 statements of the contracts in include/ptv2_hip.h; inputs: tests/gather_cases.py,
every case in two value tiers.  The bounds are derived, not measured (DESIGN.md 3.4 "Parity against float64: gather and pooling
kernels"; tests/test_gather_ref64_host.py holds an fp32 emulation to them and shows that they notice a dropped neighbour, a
shifted index row, ci / (c / w_c) for ci % w_c, a tie that goes to the last member, weights normalised by k, r % k for r / k):

    exact tier      kernel == float32(value) bit for bit, atomic scatters included
    rounding tier   |kernel - value| <= (T + 2) 2^-24 A per element (T terms, A = sum of |term|); copies, selections and
                    elements made of one term of one rounding: correctly rounded
    weights         |kernel - value| <= (k + 3) 2^-24 |value|

The launchers are called through ctypes on the current stream.  Outputs the contract does not mark [zeroed] are pre-filled
with NaN (integer outputs with a marker), the [zeroed] ones with zeros; every output is followed by a sentinel region inside the
same allocation that must come back untouched; segment_minmax's workspace is sized exactly.  The compared keys of every launcher
are asserted.  A second, shorter group goes through ao_amd.pointops.* and the _SegmentMax / _MapUnpool functions of
ao_amd/ptv2/model.py with torch.autograd.grad.

Not passed, on purpose: a negative or out-of-range id into a kernel that does not guard it (all but grouping, which skips -1,
and interpolation_weights, which rewrites it), NaN / Inf, an empty cluster (include/ptv2_hip.h: not part of pool_max's
contract)."""
import numpy as np
import pytest
import torch

from tests import gather_cases as C
from tests import gather_ref64 as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GUARD = 256            # sentinel elements behind every output
MARK_F, MARK_I = 12345.0, -77777
CALLED = set()


def _lib():
    from ao_amd import _lib as lib

    return lib


def _call(name, *args, expect=0):
    rc = getattr(_lib().lib(), name)(*args)
    CALLED.add(name)
    assert rc == expect, (name, "returned", rc, "expected", expect)


def _st():
    return _lib().stream_ptr()


def _p(t):
    return t.data_ptr()


class Buffers:
    """device arrays of one call: float arrays optionally one float off a 16-byte boundary, outputs followed by a sentinel"""

    def __init__(self, offset=False):
        self.offset, self.outs, self.keep = int(bool(offset)), [], []   # (keep: an input lives until the call has run)

    def f(self, a):
        a = np.ascontiguousarray(a, F32)
        buf = torch.empty(a.size + self.offset + 4, device="cuda")
        view = buf[self.offset:self.offset + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        self.keep.append(buf)
        assert a.size == 0 or view.data_ptr() % 16 == 4 * self.offset
        return view

    def i(self, a, pad=0):
        a = np.ascontiguousarray(a, np.int32)
        buf = torch.zeros(a.size + pad, dtype=torch.int32, device="cuda")
        buf[:a.size] = torch.from_numpy(a.ravel())
        self.keep.append(buf)
        return buf[:a.size].view(a.shape) if pad == 0 else buf

    def out(self, shape, fill, dtype=torch.float32, init=None):
        """an output of `shape` filled with `fill` (NaN: the contract writes every element; 0: [zeroed]) or holding `init`"""
        numel = int(np.prod(shape))
        off = self.offset if dtype == torch.float32 else 0
        mark = MARK_F if dtype == torch.float32 else MARK_I
        buf = torch.full((off + numel + GUARD,), mark, dtype=dtype, device="cuda")
        view = buf[off:off + numel].view(tuple(shape))
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        else:
            view.fill_(fill)
        self.outs.append((buf, off + numel, mark))
        return view

    def intact(self, what):
        for buf, end, mark in self.outs:
            assert bool((buf[end:] == mark).all()), (what, "the elements behind an output were written")


NAN = float("nan")


# -------------------------------------------------------------------------------------------------------------------- runners
def run(case, t):
    """call the case's launcher on its inputs; {output name: numpy array}"""
    name, B = case.launcher, Buffers("offset" in case.flags)
    o = {}
    if name == "grouping_forward_hip_launcher":
        m, ns = t["idx"].shape
        c = t["input"].shape[1]
        o["output"] = B.out((m, ns, c), NAN)
        _call(name, m, ns, c, _p(B.f(t["input"])), _p(B.i(t["idx"])), _p(o["output"]), _st())
    elif name == "grouping_backward_hip_launcher":
        m, ns, c = t["grad_output"].shape
        o["grad_input"] = B.out((t["n"], c), 0.0)
        _call(name, m, ns, c, _p(B.f(t["grad_output"])), _p(B.i(t["idx"])), _p(o["grad_input"]), _st())
    elif name == "interpolation_weights_hip_launcher":
        m, k = t["dist2"].shape
        o["weight"] = B.out((m, k), NAN)
        o["idx"] = B.out((m, k), 0, torch.int32, init=t["idx"])
        _call(name, m, k, t["n"], _p(B.f(t["dist2"])), _p(o["idx"]), _p(o["weight"]), _st())
    elif name == "interpolation_forward_hip_launcher":
        n, k = t["idx"].shape
        c = t["input"].shape[1]
        o["output"] = B.out((n, c), 0.0)
        _call(name, n, c, k, _p(B.f(t["input"])), _p(B.i(t["idx"])), _p(B.f(t["weight"])), _p(o["output"]), _st())
    elif name == "interpolation_backward_hip_launcher":
        n, k = t["idx"].shape
        c = t["grad_output"].shape[1]
        o["grad_input"] = B.out((t["m"], c), 0.0)
        _call(name, n, c, k, _p(B.f(t["grad_output"])), _p(B.i(t["idx"])), _p(B.f(t["weight"])), _p(o["grad_input"]), _st())
    elif name == "interpolation_backward_gather_hip_launcher":
        n, k = t["idx"].shape
        c = t["grad_output"].shape[1]
        assert t["m"] <= max(n, 1)
        inv_ptr, inv_rows = R.inverse_table(t["idx"], t["m"])
        o["grad_input"] = B.out((t["m"], c), NAN)          # fully written: rows nobody points at get zeros
        _call(name, t["m"], c, k, _p(B.f(t["grad_output"])), _p(B.i(inv_ptr)), _p(B.i(inv_rows, pad=4)), _p(B.f(t["weight"])),
              _p(o["grad_input"]), _st())
    elif name == "subtraction_forward_hip_launcher":
        n, ns = t["idx"].shape
        c = t["input1"].shape[1]
        o["output"] = B.out((n, ns, c), NAN)
        _call(name, n, ns, c, _p(B.f(t["input1"])), _p(B.f(t["input2"])), _p(B.i(t["idx"])), _p(o["output"]), _st())
    elif name == "subtraction_backward_hip_launcher":
        n, ns, c = t["grad_output"].shape
        o["grad_input1"], o["grad_input2"] = B.out((n, c), 0.0), B.out((n, c), 0.0)
        _call(name, n, ns, c, _p(B.i(t["idx"])), _p(B.f(t["grad_output"])), _p(o["grad_input1"]), _p(o["grad_input2"]), _st())
    elif name == "aggregation_forward_hip_launcher":
        n, ns, c = t["position"].shape
        w_c = t["weight"].shape[2]
        o["output"] = B.out((n, c), 0.0)
        _call(name, n, ns, c, w_c, _p(B.f(t["input"])), _p(B.f(t["position"])), _p(B.f(t["weight"])), _p(B.i(t["idx"])),
              _p(o["output"]), _st())
    elif name == "aggregation_backward_hip_launcher":
        n, ns, c = t["position"].shape
        w_c = t["weight"].shape[2]
        o["grad_input"] = B.out((t["input"].shape[0], c), 0.0)
        o["grad_position"] = B.out((n, ns, c), NAN)        # not [zeroed] in the header: every element is written
        o["grad_weight"] = B.out((n, ns, w_c), 0.0)
        _call(name, n, ns, c, w_c, _p(B.f(t["input"])), _p(B.f(t["position"])), _p(B.f(t["weight"])), _p(B.i(t["idx"])),
              _p(B.f(t["grad_output"])), _p(o["grad_input"]), _p(o["grad_position"]), _p(o["grad_weight"]), _st())
    elif name == "attention_relation_step_forward_hip_launcher":
        m, (n, g, c) = t["index_target"].shape[0], t["query"].shape
        o["output"] = B.out((m, g), 0.0)
        _call(name, m, g, c, _p(B.f(t["query"])), _p(B.f(t["key"])), _p(B.f(t["weight"])), _p(B.i(t["index_target"])),
              _p(B.i(t["index_refer"])), _p(o["output"]), _st())
    elif name == "attention_relation_step_backward_hip_launcher":
        m, (n, g, c) = t["index_target"].shape[0], t["query"].shape
        o["grad_query"], o["grad_key"], o["grad_weight"] = B.out((n, g, c), 0.0), B.out((n, g, c), 0.0), B.out((c,), 0.0)
        _call(name, m, g, c, _p(B.f(t["query"])), _p(o["grad_query"]), _p(B.f(t["key"])), _p(o["grad_key"]), _p(B.f(t["weight"])),
              _p(o["grad_weight"]), _p(B.i(t["index_target"])), _p(B.i(t["index_refer"])), _p(B.f(t["grad_output"])), _st())
    elif name == "attention_fusion_step_forward_hip_launcher":
        m, (n, g, c) = t["index_target"].shape[0], t["value"].shape
        o["output"] = B.out((n, g, c), 0.0)
        _call(name, m, g, c, _p(B.f(t["weight"])), _p(B.f(t["value"])), _p(B.i(t["index_target"])), _p(B.i(t["index_refer"])),
              _p(o["output"]), _st())
    elif name == "attention_fusion_step_backward_hip_launcher":
        m, (n, g, c) = t["index_target"].shape[0], t["value"].shape
        o["grad_weight"], o["grad_value"] = B.out((m, g), 0.0), B.out((n, g, c), 0.0)
        _call(name, m, g, c, _p(B.f(t["weight"])), _p(o["grad_weight"]), _p(B.f(t["value"])), _p(o["grad_value"]),
              _p(B.i(t["index_target"])), _p(B.i(t["index_refer"])), _p(B.f(t["grad_output"])), _st())
    elif name == "segment_minmax_hip_launcher":
        b = t["offset"].size
        nbytes = int(_lib().lib().segment_minmax_hip_workspace_bytes(b))
        CALLED.add("segment_minmax_hip_workspace_bytes")
        ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device="cuda")   # exactly nbytes, then a sentinel
        o["lo"], o["hi"] = B.out((b, 3), NAN), B.out((b, 3), NAN)
        _call(name, b, _p(B.f(t["xyz"])), _p(B.i(t["offset"])), _p(o["lo"]), _p(o["hi"]), _p(ws), nbytes, _st())
        _call(name, b, _p(B.f(t["xyz"])), _p(B.i(t["offset"])), _p(o["lo"]), _p(o["hi"]), _p(ws), nbytes - 1, _st(), expect=2)
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), "the bytes behind the workspace were written"
    elif name == "pool_max_forward_hip_launcher":
        n_out, c = t["idx_ptr"].size - 1, t["feat"].shape[1]
        o["out"], o["arg"] = B.out((n_out, c), NAN), B.out((n_out, c), MARK_I, torch.int32)
        _call(name, n_out, c, _p(B.f(t["feat"])), _p(B.i(t["order"])), _p(B.i(t["idx_ptr"])), _p(o["out"]), _p(o["arg"]), _st())
    elif name == "pool_max_backward_hip_launcher":
        n_out, c = t["grad_out"].shape
        o["grad_feat"] = B.out((t["n_in"], c), 0.0)
        _call(name, n_out, c, _p(B.f(t["grad_out"])), _p(B.i(t["arg"])), _p(o["grad_feat"]), _st())
    elif name == "segment_sum_hip_launcher":
        n_out, c = t["idx_ptr"].size - 1, t["grad_fine"].shape[1]
        o["grad_coarse"] = B.out((n_out, c), NAN)
        _call(name, n_out, c, _p(B.f(t["grad_fine"])), _p(B.i(t["order"])), _p(B.i(t["idx_ptr"])), _p(o["grad_coarse"]), _st())
    else:
        raise AssertionError(name)
    torch.cuda.synchronize()
    B.intact((name, case.name))
    return {k: v.cpu().numpy() for k, v in o.items()}


def check(case, tier):
    t, ref, _ = C.inputs(case, tier)
    got = run(case, t)
    name = case.launcher
    assert set(got) == set(R.KEYS[name]) == set(ref), (name, sorted(got), sorted(ref))
    failures = []
    for key in R.KEYS[name]:
        if name == "interpolation_weights_hip_launcher" and key == "weight" and tier == "rounding":
            ok, ratio, msg = R.compare_weights(got[key], ref[key], case.p["ns"])
        else:
            ok, ratio, msg = R.compare(got[key], ref[key], tier)
        if tier == "rounding":
            print("gather-ratio %s %s %s worst err/bound %.4f" % (name, key, case.name, ratio))
        if not ok:
            failures.append((key, ratio, msg))
    assert not failures, (name, case.name, tier, failures)


def _params(launcher):
    return [pytest.param(case, tier, id="%s-%s" % (case.name, tier)) for case, tier in C.pairs(launcher)]


@pytest.mark.parametrize("case,tier", _params("grouping_forward_hip_launcher"))
def test_grouping_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("grouping_backward_hip_launcher"))
def test_grouping_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("interpolation_weights_hip_launcher"))
def test_interpolation_weights(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("interpolation_forward_hip_launcher"))
def test_interpolation_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("interpolation_backward_hip_launcher"))
def test_interpolation_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("interpolation_backward_gather_hip_launcher"))
def test_interpolation_backward_gather(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("subtraction_forward_hip_launcher"))
def test_subtraction_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("subtraction_backward_hip_launcher"))
def test_subtraction_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("aggregation_forward_hip_launcher"))
def test_aggregation_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("aggregation_backward_hip_launcher"))
def test_aggregation_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("attention_relation_step_forward_hip_launcher"))
def test_attention_relation_step_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("attention_relation_step_backward_hip_launcher"))
def test_attention_relation_step_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("attention_fusion_step_forward_hip_launcher"))
def test_attention_fusion_step_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("attention_fusion_step_backward_hip_launcher"))
def test_attention_fusion_step_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("segment_minmax_hip_launcher"))
def test_segment_minmax(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("pool_max_forward_hip_launcher"))
def test_pool_max_forward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("pool_max_backward_hip_launcher"))
def test_pool_max_backward(case, tier):
    check(case, tier)


@pytest.mark.parametrize("case,tier", _params("segment_sum_hip_launcher"))
def test_segment_sum(case, tier):
    check(case, tier)


def test_interpolation_weights_refuses_k_0_and_k_9_without_a_launch():
    B = Buffers()
    d2, idx = B.f(np.ones((4, 9), F32)), B.out((4, 9), 0, torch.int32, init=np.full((4, 9), -1, np.int32))
    w = B.out((4, 9), NAN)
    for k in (0, 9):
        _call("interpolation_weights_hip_launcher", 4, k, 50, _p(d2), _p(idx), _p(w), _st(), expect=1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(w).all()) and bool((idx == -1).all())
    B.intact("interpolation_weights refusals")


# atomics-free launchers: two identical calls give the same bits
FIXED_ORDER = ("grouping_forward_hip_launcher", "interpolation_weights_hip_launcher", "interpolation_forward_hip_launcher",
               "interpolation_backward_gather_hip_launcher", "subtraction_forward_hip_launcher", "aggregation_forward_hip_launcher",
               "attention_relation_step_forward_hip_launcher", "segment_minmax_hip_launcher", "pool_max_forward_hip_launcher",
               "pool_max_backward_hip_launcher", "segment_sum_hip_launcher")


@pytest.mark.parametrize("launcher", FIXED_ORDER)
def test_atomics_free_launchers_repeat_their_bits(launcher):
    case = next(c for c in C.CASES[launcher] if C.threads(c) > 200 and "big" not in c.flags)
    t, _, _ = C.inputs(case, "rounding")
    a, b = run(case, t), run(case, t)
    assert set(a) == set(R.KEYS[launcher])
    for key in a:
        assert R.bits_equal(a[key], b[key]), (launcher, case.name, key)


# --------------------------------------------------------------------------------------------------------- the python API
def _cuda(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return x.requires_grad_(True) if grad else x


def _hold(what, got, ref, tier="rounding"):
    assert got.dtype == torch.float32, (what, got.dtype)
    ok, ratio, msg = R.compare(got.detach().cpu().numpy(), ref, tier)
    print("gather-ratio api %s worst err/bound %.4f" % (what, ratio))
    assert ok, (what, ratio, msg)


def _inputs(launcher, pick, tier="rounding"):
    return C.inputs(C.CASES[launcher][pick], tier)


class _Spy:
    """the ctypes library with the launcher names it was asked for"""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.real, name)


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(_lib().lib())
    monkeypatch.setattr(_lib(), "lib", lambda: s)
    return s


@pytest.mark.parametrize("pick", [4, 5])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-bf16"])
def test_pointops_api_against_float64(pick, autocast, spy):
    """ao_amd.pointops.{grouping2, subtraction, aggregation, attention_relation_step, attention_fusion_step}: forward and
    torch.autograd.grad against the statements.  Under torch.autocast(bfloat16) the ops run in fp32 on the fp32 inputs
    (custom_fwd casts to float32) and return fp32: the same bounds hold."""
    from ao_amd import pointops as hp

    rng = np.random.default_rng(pick)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        t, ref, _ = _inputs("grouping_forward_hip_launcher", pick)
        x = _cuda(t["input"], True)
        out = hp.grouping2(x, _cuda(t["idx"]))
        _hold("grouping2", out, ref["output"])
        go = rng.standard_normal(out.shape).astype(F32)
        (gx,) = torch.autograd.grad(out, x, _cuda(go))
        _hold("grouping2 grad", gx, R.grouping_backward(dict(grad_output=go, idx=t["idx"], n=t["input"].shape[0]))["grad_input"])

        t, ref, _ = _inputs("subtraction_forward_hip_launcher", pick)
        a, b = _cuda(t["input1"], True), _cuda(t["input2"], True)
        out = hp.subtraction(a, b, _cuda(t["idx"]))
        _hold("subtraction", out, ref["output"])
        go = rng.standard_normal(out.shape).astype(F32)
        ga, gb = torch.autograd.grad(out, (a, b), _cuda(go))
        back = R.subtraction_backward(dict(grad_output=go, idx=t["idx"]))
        _hold("subtraction grad 1", ga, back["grad_input1"])
        _hold("subtraction grad 2", gb, back["grad_input2"])

        t, ref, _ = _inputs("aggregation_backward_hip_launcher", pick)
        x, p, w = (_cuda(t[k], True) for k in ("input", "position", "weight"))
        out = hp.aggregation(x, p, w, _cuda(t["idx"]))
        _hold("aggregation", out, R.aggregation_forward(t)["output"])
        for got, key in zip(torch.autograd.grad(out, (x, p, w), _cuda(t["grad_output"])), ("grad_input", "grad_position", "grad_weight")):
            _hold("aggregation " + key, got, ref[key])

        t, ref, _ = _inputs("attention_relation_step_backward_hip_launcher", pick - 1)
        q, k = _cuda(t["query"], True), _cuda(t["key"], True)
        out = hp.attention_relation_step(q, k, _cuda(t["weight"]), _cuda(t["index_target"]), _cuda(t["index_refer"]))
        _hold("relation", out, R.attention_relation_step_forward(t)["output"])
        gq, gk = torch.autograd.grad(out, (q, k), _cuda(t["grad_output"]))
        _hold("relation grad_query", gq, ref["grad_query"])
        _hold("relation grad_key", gk, ref["grad_key"])

        t, ref, _ = _inputs("attention_fusion_step_backward_hip_launcher", pick - 1)
        w, v = _cuda(t["weight"], True), _cuda(t["value"], True)
        out = hp.attention_fusion_step(w, v, _cuda(t["index_target"]), _cuda(t["index_refer"]))
        _hold("fusion", out, R.attention_fusion_step_forward(t)["output"])
        gw, gv = torch.autograd.grad(out, (w, v), _cuda(t["grad_output"]))
        _hold("fusion grad_weight", gw, ref["grad_weight"])
        _hold("fusion grad_value", gv, ref["grad_value"])
    want = {n for n in R.CONTRACTS if n.startswith(("grouping", "subtraction", "aggregation", "attention"))}
    assert want <= set(spy.names), sorted(want - set(spy.names))


@pytest.mark.parametrize("pick", [4, 5])
@pytest.mark.parametrize("route", ["gather", "atomic-no-table", "atomic-stale-table", "atomic-m-above-n"])
def test_interpolation_api_takes_the_gather_backward_only_with_a_valid_inverse(pick, route, spy):
    """_InterpolateRows: the gather backward when idx carries a valid _ao_inverse and m <= n, the atomic one otherwise; both give
    the reference gradient"""
    from ao_amd.pointops.interpolation import _InterpolateRows

    t, ref, _ = _inputs("interpolation_backward_hip_launcher", pick)
    n, m = t["idx"].shape[0], t["m"]
    if route == "atomic-m-above-n":   # more coarse rows than fine ones: the first 40 fine rows only
        t = dict(t, idx=t["idx"][:40], weight=t["weight"][:40], grad_output=t["grad_output"][:40])
        assert m > 40
        ref = R.interpolation_backward(t)
    rng = np.random.default_rng(pick)
    feat = _cuda(rng.standard_normal((m, t["grad_output"].shape[1])).astype(F32), True)
    idx, weight = _cuda(t["idx"]), _cuda(t["weight"])
    if route != "atomic-no-table":
        inv_ptr, inv_rows = R.inverse_table(t["idx"], m)
        idx._ao_inverse = (idx._version - (route == "atomic-stale-table"), _cuda(inv_ptr), _cuda(inv_rows))
    out = _InterpolateRows.apply(feat, idx, weight)
    _hold("interpolation " + route, out, R.interpolation_forward(dict(input=feat.detach().cpu().numpy(), idx=t["idx"],
                                                                       weight=t["weight"]))["output"])
    (gf,) = torch.autograd.grad(out, feat, _cuda(t["grad_output"]))
    _hold("interpolation grad " + route, gf, ref["grad_input"])
    gather = "interpolation_backward_gather_hip_launcher" in spy.names
    atomic = "interpolation_backward_hip_launcher" in spy.names
    assert (gather, atomic) == ((True, False) if route == "gather" else (False, True)), (route, spy.names)


def test_interpolation_api_under_autocast_returns_fp32(spy):
    from ao_amd.pointops.interpolation import _InterpolateRows

    t, ref, _ = _inputs("interpolation_backward_hip_launcher", 4)
    feat = _cuda(np.random.default_rng(0).standard_normal((t["m"], t["grad_output"].shape[1])).astype(F32), True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = _InterpolateRows.apply(feat, _cuda(t["idx"]), _cuda(t["weight"]))
        (gf,) = torch.autograd.grad(out, feat, _cuda(t["grad_output"]))
    assert out.dtype == torch.float32
    _hold("interpolation grad autocast", gf, ref["grad_input"])


@pytest.mark.parametrize("pick", [5, 12])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-bf16"])
def test_segment_max_and_map_unpool_against_float64(pick, autocast, spy):
    """_SegmentMax (pool_max forward / backward) and _MapUnpool (segment_sum) of ao_amd/ptv2/model.py"""
    from ao_amd.ptv2.model import _MapUnpool, _SegmentMax

    t, ref, _ = _inputs("pool_max_forward_hip_launcher", pick)
    rng = np.random.default_rng(pick)
    n_in, (n_out, c) = t["feat"].shape[0], ref["out"].shape
    order, ptr = _cuda(t["order"]), _cuda(t["idx_ptr"])
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        feat = _cuda(t["feat"], True)
        out = _SegmentMax.apply(feat, order, ptr)
        _hold("segment_max", out, ref["out"])
        go = rng.standard_normal((n_out, c)).astype(F32)
        (gf,) = torch.autograd.grad(out, feat, _cuda(go))
        _hold("segment_max grad", gf, R.pool_max_backward(dict(grad_out=go, arg=ref["arg"], n_in=n_in))["grad_feat"])

        cluster = np.empty(n_in, np.int64)
        cluster[t["order"]] = np.repeat(np.arange(n_out), np.diff(t["idx_ptr"]))
        coarse = _cuda(rng.standard_normal((n_out, c)).astype(F32), True)
        fine = _MapUnpool.apply(coarse, _cuda(cluster), order, ptr)
        assert torch.equal(fine, coarse.detach()[_cuda(cluster)])
        gfine = rng.standard_normal((n_in, c)).astype(F32)
        (gc,) = torch.autograd.grad(fine, coarse, _cuda(gfine))
        _hold("map_unpool grad", gc, R.segment_sum(dict(grad_fine=gfine, order=t["order"], idx_ptr=t["idx_ptr"]))["grad_coarse"])
    assert {"pool_max_forward_hip_launcher", "pool_max_backward_hip_launcher", "segment_sum_hip_launcher"} <= set(spy.names)


# ---------------------------------------------------------------------------------------------------------------------- coverage
def test_every_gather_and_pooling_launcher_is_called_directly():
    """a tour over one case of every launcher, then the names called against the 18 of the two kernel files (and the header
    declares each of them)"""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptv2_hip.h")) as f:
        header = f.read()
    CALLED.clear()
    for launcher, cases in C.CASES.items():
        check(next(c for c in cases if C.threads(c) > 1000 and "big" not in c.flags), "exact" if "weights" not in launcher else "rounding")
    want = set(R.CONTRACTS)
    assert len(want) == 18 and all("int %s(" % name in header for name in want)
    assert CALLED == want | {"segment_minmax_hip_workspace_bytes"}, (sorted(want - CALLED), sorted(CALLED - want))
