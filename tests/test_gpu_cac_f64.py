"""GPU: the six launchers of ao_amd/csrc/cac.hip (with cac_workspace_bytes its seven entry points) and the two of
ao_amd/csrc/loss.hip against float64, one launcher per call.

Reference: tests/cac_ref64.py -- float64 statements of the contracts in include/ptv2_hip.h, each output with the bound that follows
from its operations (sum lengths, one unit per rounding, four units in the last place per expf / logf / sqrtf / division, the
error of an inner quantity carried into the outer one); nothing in it is measured on a kernel.  Inputs: tests/cac_cases.py, every
case in a plain and a wide value tier.  tests/test_cac_ref64_host.py holds an fp32 emulation to the same bounds in three summation
orders and shows that they notice a dropped tile row, a dropped slab, class k read as k - 64, an inverted mask, label -1 counted as
class 0, a cosine normalised by |x|^2, an ignored row with entropy weight 1 and a cross-entropy averaged over n.  Exact outputs
(mode 1's z, the distillation's row counts, count, bad_labels, gradients of ignored rows, the all-ignored loss) compare bit for bit.

The launchers are called through ctypes on the current stream.  Outputs are pre-filled with NaN and followed by a sentinel region
inside the same allocation that must come back untouched; workspaces are sized exactly by cac_workspace_bytes /
cross_entropy_workspace_bytes and followed by a sentinel too.  The backward launchers take z, out, lse, coef and count from the
kernel's own forward, as the autograd functions do.  The compared outputs of every launcher and the set of launchers called are
asserted.  A shorter group goes through _WeightedSum, _Cosine, _Distill and ao_amd.ptv2.segmentor.cross_entropy with
torch.autograd.grad.  Every (case, tier) prints the worst err / bound of each output; DESIGN.md 3.8c records them.

Not passed, on purpose: NaN or Inf inputs; a max_rows below the largest scene; rows beyond offset[b - 1]; labels outside [0, K)
other than -1 into the CAC kernels (the header does not define them)."""
import faulthandler
import os

import numpy as np
import pytest
import torch

from tests import cac_cases as C
from tests import cac_ref64 as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GUARD = 256            # sentinel elements behind every output
PAD = 4096             # sentinel bytes behind a workspace
MARK = 12345.0
ERR_ARG, ERR_WORKSPACE = 1, 2
CALLED = set()
WORST = {}

WSF, WSB = "cac_weighted_sum_forward_hip_launcher", "cac_weighted_sum_backward_hip_launcher"
COF, COB = "cac_cosine_forward_hip_launcher", "cac_cosine_backward_hip_launcher"
DIF, DIB = "cac_distill_forward_hip_launcher", "cac_distill_backward_hip_launcher"
CEF, CEB = "cross_entropy_forward_hip_launcher", "cross_entropy_backward_hip_launcher"


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the card"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _lib():
    from ao_amd import _lib as lib

    return lib


def _call(name, *args, expect=0):
    rc = getattr(_lib().lib(), name)(*args)
    CALLED.add(name)
    assert rc == expect, (name, "returned", rc, "expected", expect)


def _bytes(name, *args):
    CALLED.add(name)
    return int(getattr(_lib().lib(), name)(*args))


def _st():
    return _lib().stream_ptr()


def _p(t):
    return 0 if t is None else t.data_ptr()


def align256(v):
    return (v + 255) // 256 * 256


class Buffers:
    """device arrays of one call: outputs NaN-filled and followed by a sentinel, workspaces of an exact size followed by one"""

    def __init__(self):
        self.outs, self.spaces = [], []

    @staticmethod
    def f(a):
        return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()

    @staticmethod
    def l(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()

    @staticmethod
    def i(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()

    def out(self, shape):
        numel = int(np.prod(shape))
        buf = torch.full((numel + GUARD,), MARK, dtype=torch.float32, device="cuda")
        view = buf[:numel].view(tuple(shape))
        view.fill_(float("nan"))
        self.outs.append((buf, numel))
        return view

    def ws(self, nbytes):
        buf = torch.full((nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.spaces.append((buf, nbytes))
        return buf

    def intact(self, what):
        for buf, end in self.outs:
            assert bool((buf[end:] == MARK).all()), (what, "the elements behind an output were written")
        for buf, end in self.spaces:
            assert bool((buf[end:] == 0xA5).all()), (what, "the bytes behind the workspace were written")


# -------------------------------------------------------------------------------------------------------------------- runners
def run(launcher, case, tier, short=0, **var):
    """call `launcher` on the case (a backward after the kernel's own forward); {output name: numpy array}.  `short`: bytes taken
    off the exact workspace of the launcher under test, which must then refuse"""
    exact = var.pop("exact", False)
    t, full, B, o = C.view(case, tier, launcher, **var), C.inputs(case, tier), Buffers(), {}
    refuse = dict(expect=ERR_WORKSPACE) if short else {}
    if launcher in (WSF, WSB):
        mode, (n, c), k, b, rows = t["mode"], t["x"].shape, t["k"], full["b"], full["max_rows"]
        x, off = B.f(t["x"]), B.i(t["offset"])
        logits, label = (B.f(t["logits"]), None) if mode == 0 else (None, B.l(t["label"]))
        sets = b if mode == 0 else 1
        z, out = B.out((sets, k)), B.out((sets, k, c))
        nbytes = _bytes("cac_workspace_bytes", b, rows, n, k, c)
        ws = B.ws(nbytes - short)
        _call(WSF, mode, n, b, rows, k, c, _p(x), _p(logits), _p(label), _p(off), t["thr"], t["eps"], _p(z), _p(out), _p(ws),
              nbytes - short, _st(), **refuse)
        o = dict(z=z, out=out)
        if launcher == WSB:
            dout, gx = B.f(t["dout"]), B.out((n, c))
            gl = B.out((n, k)) if t["glogits"] else None
            _call(WSB, mode, n, b, rows, k, c, _p(x), _p(logits), _p(label), _p(off), t["thr"], t["eps"], _p(z), _p(out), _p(dout),
                  _p(gx), _p(gl), _st())
            o = dict(gx=gx, glogits=gl) if gl is not None else dict(gx=gx)
    elif launcher in (COF, COB):
        (n, c), k, b, rows = t["x"].shape, t["k"], full["b"], full["max_rows"]
        x, q, off = B.f(t["x"]), B.f(t["q"]), B.i(t["offset"])
        if launcher == COF:
            o = dict(out=B.out((n, k)))
            _call(COF, n, b, rows, k, c, _p(x), _p(q), t["per_scene"], _p(off), t["scale"], _p(o["out"]), _st())
        else:
            o = dict(gx=B.out((n, c)), gq=B.out(t["q"].shape))
            nbytes = _bytes("cac_workspace_bytes", b, rows, n, k, c)
            ws = B.ws(nbytes - short)
            _call(COB, n, b, rows, k, c, _p(x), _p(q), t["per_scene"], _p(off), t["scale"], _p(B.f(t["dout"])), _p(o["gx"]),
                  _p(o["gq"]), _p(ws), nbytes - short, _st(), **refuse)
    elif launcher in (DIF, DIB):
        n, k = t["pred"].shape
        pred, soft, label = B.f(t["pred"]), B.f(t["soft"]), B.l(t["label"])
        loss, coef = B.out((1,)), B.out((k,))
        # the public size (as _Distill asks for it), or with exact=True the launcher's own need: the partials, then 3 k sums
        # at the next 256-byte boundary
        sums_at = align256(4 * 3 * k * -(-n // R.CHUNK))
        nbytes = sums_at + 4 * 3 * k if exact or short else _bytes("cac_workspace_bytes", 1, 1, n, k, 4)
        ws = B.ws(nbytes - short)
        _call(DIF, n, k, _p(pred), _p(soft), _p(label), _p(loss), _p(coef), _p(ws), nbytes - short, _st(), **refuse)
        o = dict(loss=loss, coef=coef)
        if not short:
            o["rows"] = ws[sums_at:sums_at + 4 * 3 * k].view(torch.float32)[2 * k:].clone()
        if launcher == DIB:
            o = dict(gpred=B.out((n, k)))
            _call(DIB, n, k, _p(pred), _p(soft), _p(label), _p(coef), _p(B.f([t["g"]])), _p(o["gpred"]), _st())
    elif launcher in (CEF, CEB):
        n, c = t["logits"].shape
        logits, label = B.f(t["logits"]), B.l(t["label"])
        o = dict(lse=B.out((n,)), loss=B.out((1,)), count=B.out((1,)), bad_labels=B.out((1,)))
        nbytes = _bytes("cross_entropy_workspace_bytes", n)
        ws = B.ws(nbytes - short)
        _call(CEF, n, c, _p(logits), _p(label), t["ignore_index"], _p(o["lse"]), _p(o["loss"]), _p(o["count"]), _p(o["bad_labels"]),
              _p(ws), nbytes - short, _st(), **refuse)
        if launcher == CEB:
            lse, count = o["lse"], o["count"]
            o = dict(g_logits=B.out((n, c)))
            _call(CEB, n, c, _p(logits), _p(label), t["ignore_index"], _p(lse), _p(B.f([t["g"]])), _p(count), _p(o["g_logits"]), _st())
    else:
        raise AssertionError(launcher)
    torch.cuda.synchronize()
    B.intact((launcher, case.name, tier, var))
    return {key: v.cpu().numpy() for key, v in o.items()}


def hold(what, got, ref):
    """every output of `got` against the statement's: the failures of all of them in one assertion"""
    failures = []
    for key in ref:
        ok, ratio, msg = R.compare(got[key], ref[key])
        print("cac-ratio %s %s worst err/bound %.4f" % (" ".join(str(w) for w in what), key, ratio))
        slot = (what[1] if what[0] == "api" else what[0], key)
        if np.isfinite(ratio) and ratio >= WORST.get(slot, (-1.0, ""))[0]:
            WORST[slot] = (ratio, " ".join(str(w) for w in what[1:]))
        if not ok:
            failures.append((key, ratio, msg))
    assert not failures, (what, failures)


def check(launcher, case, tier):
    for var in C.variants(case, launcher):
        ref = C.reference(case, tier, launcher, **var)
        got = run(launcher, case, tier, **var)
        want = set(R.KEYS[launcher]) - ({"glogits"} if launcher == WSB and not (var.get("mode") == 0 and var.get("glogits", True))
                                       else set())
        assert set(got) == want == set(ref), (launcher, var, sorted(got), sorted(ref))
        hold((launcher, case.name, tier, "".join("%s%d" % (k[0], v) for k, v in sorted(var.items()))), got, ref)


def _params(launcher):
    return [pytest.param(case, tier, id="%s-%s" % (case.name, tier)) for case, tier in C.pairs(C.FAMILY[launcher])]


@pytest.mark.parametrize("case,tier", _params(WSF))
def test_weighted_sum_forward(case, tier):
    check(WSF, case, tier)


@pytest.mark.parametrize("case,tier", _params(WSB))
def test_weighted_sum_backward(case, tier):
    check(WSB, case, tier)


@pytest.mark.parametrize("case,tier", _params(COF))
def test_cosine_forward(case, tier):
    check(COF, case, tier)


@pytest.mark.parametrize("case,tier", _params(COB))
def test_cosine_backward(case, tier):
    check(COB, case, tier)


@pytest.mark.parametrize("case,tier", _params(DIF))
def test_distill_forward(case, tier):
    check(DIF, case, tier)
    if case.p["layout"] == "allign":   # no labelled row: the loss is 0 and no class has a coefficient, exactly
        got = run(DIF, case, tier)
        assert not got["loss"].any() and not got["coef"].any() and not got["rows"].any()


@pytest.mark.parametrize("case,tier", _params(DIB))
def test_distill_backward(case, tier):
    check(DIB, case, tier)
    got = run(DIB, case, tier)["gpred"]
    assert not got[C.inputs(case, tier)["label"] == -1].any()   # an ignored row: zero, exactly


@pytest.mark.parametrize("case,tier", _params(CEF))
def test_cross_entropy_forward(case, tier):
    check(CEF, case, tier)
    if "bad" in case.flags:
        got = run(CEF, case, tier)
        assert np.isnan(got["loss"]).all() and got["bad_labels"][0] == 1.0


@pytest.mark.parametrize("case,tier", _params(CEB))
def test_cross_entropy_backward(case, tier):
    check(CEB, case, tier)
    t = C.inputs(case, tier)
    got = run(CEB, case, tier)["g_logits"]
    assert not got[t["label"] == t["ignore_index"]].any()        # an ignored row: zero, exactly


# --------------------------------------------------------------------------------------------------------------------- guards
def _scene(name):
    return next(c for c in C.CASES["scene"] if c.name == name)


def test_refusals_return_before_a_launch():
    """C = 6, K = 257, K = 0 and a null required pointer: PTV2_ERR_ARG, and nothing is written"""
    B = Buffers()
    n, b, k, c = 40, 1, 20, 8
    x, logits, label, off = B.f(np.ones((n, c))), B.f(np.ones((n, k))), B.l(np.zeros(n)), B.i([n])
    big = B.out((4 * 257 * 64,))          # stands for every output; nothing may be written into it
    ws = B.ws(1 << 20)
    g = B.f([1.0])
    for kk, cc, nul in ((k, 6, 0), (257, c, 0), (0, c, 0), (k, c, 1)):
        xx = 0 if nul else _p(x)
        for mode in (0, 1):
            _call(WSF, mode, n, b, n, kk, cc, xx, _p(logits), _p(label), _p(off), 0.0, 1e-7, _p(big), _p(big), _p(ws), 1 << 20, _st(),
                  expect=ERR_ARG)
            _call(WSB, mode, n, b, n, kk, cc, xx, _p(logits), _p(label), _p(off), 0.0, 1e-7, _p(big), _p(big), _p(big), _p(big), 0,
                  _st(), expect=ERR_ARG)
        _call(COF, n, b, n, kk, cc, xx, _p(big), 1, _p(off), 15.0, _p(big), _st(), expect=ERR_ARG)
        _call(COB, n, b, n, kk, cc, xx, _p(big), 1, _p(off), 15.0, _p(big), _p(big), _p(big), _p(ws), 1 << 20, _st(), expect=ERR_ARG)
        if cc == c:
            pred = 0 if nul else _p(logits)
            _call(DIF, n, kk, pred, _p(logits), _p(label), _p(big), _p(big), _p(ws), 1 << 20, _st(), expect=ERR_ARG)
            _call(DIB, n, kk, pred, _p(logits), _p(label), _p(big), _p(g), _p(big), _st(), expect=ERR_ARG)
    _call(WSB, 1, n, b, n, k, c, _p(x), 0, _p(label), _p(off), 0.0, 1e-4, _p(big), _p(big), _p(big), _p(big), _p(big), _st(),
          expect=ERR_ARG)             # glogits asked of mode 1
    _call(CEF, n, 0, _p(logits), _p(label), -1, _p(big), _p(big), _p(big), _p(big), _p(ws), 1 << 20, _st(), expect=ERR_ARG)
    _call(CEF, n, k, 0, _p(label), -1, _p(big), _p(big), _p(big), _p(big), _p(ws), 1 << 20, _st(), expect=ERR_ARG)
    _call(CEB, n, k, _p(logits), 0, -1, _p(big), _p(g), _p(g), _p(big), _st(), expect=ERR_ARG)
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all())
    B.intact("refusals")


@pytest.mark.parametrize("launcher,family,name", [(WSF, "scene", "k20-c48-r257-thr0"), (COB, "scene", "k20-c48-r257-thr0"),
                                                  (DIF, "distill", "k20-n257-all"), (CEF, "ce", "c13-n257-ig0-ii-1")])
def test_workspace_one_byte_short_is_refused_and_the_exact_need_runs(launcher, family, name):
    """the distillation's need is the layout it guards: align256(partials) + 3 k floats = 752 bytes at k = 20, n = 257"""
    case = next(c for c in C.CASES[family] if c.name == name)
    var = C.variants(case, launcher)[0]
    got = run(launcher, case, "plain", short=1, **var)
    assert all(np.isnan(v).all() for v in got.values()), "a refused call wrote an output"
    exact = dict(var, exact=True) if launcher == DIF else var
    got = run(launcher, case, "plain", **exact)            # (run() checks the bytes behind the exactly sized workspace)
    hold((launcher, case.name, "plain", "exact-workspace"), got, C.reference(case, "plain", launcher, **var))


def test_distill_need_is_the_layout():
    assert align256(4 * 3 * 20 * 2) + 4 * 3 * 20 == 752


# ---------------------------------------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("launcher,family,name", [
    (WSB, "scene", "k65-c8-s3x1000-thr0"), (WSF, "scene", "k20-c48-r2305-thr075"), (COF, "scene", "k20-c48-s3x1000-thr075"),
    (COB, "scene", "k20-c48-s3x1000-thr075"), (DIB, "distill", "k20-n16385-ign30"), (DIF, "distill", "k65-n16385-ign30"),
    (CEB, "ce", "c13-n257-ig0.1-ii255"), (CEF, "ce", "c13-n262401-ig0.1-ii-1-stride")])
def test_a_second_identical_call_gives_the_same_bits(launcher, family, name):
    """ao_amd/csrc/cac.hip: "Results are bitwise reproducible from run to run" (fixed-order slabs, no float atomics); the
    cross-entropy's last block adds the partials in a fixed tree"""
    case = next(c for c in C.CASES[family] if c.name == name)
    for var in C.variants(case, launcher):
        a, b = run(launcher, case, "plain", **var), run(launcher, case, "plain", **var)
        assert set(a) == set(b)
        for key in a:
            assert R.bits_equal(a[key], b[key]), (launcher, case.name, var, key)


# ------------------------------------------------------------------------------------------------------------- through autograd
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


def _cuda(a, grad=False, strided=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if strided:   # the same values behind a transposed layout: the functions have to make it contiguous
        x = x.t().contiguous().t()
        assert not x.is_contiguous() or min(x.shape) == 1
    return x.requires_grad_(True) if grad else x


def _api(what, got, ref):
    hold(("api",) + what, {k: v.detach().cpu().numpy() for k, v in got.items()}, {k: ref[k] for k in got})


@pytest.mark.parametrize("name", ["k20-c48-s300_0_17-thr075", "k65-c8-r257-thr0", "k200-c48-r17-thr075"])
@pytest.mark.parametrize("tier", C.TIERS)
def test_weighted_sum_and_cosine_through_autograd(name, tier, spy):
    """_WeightedSum (both modes; the logits' gradient asked for, and not asked for as under detach_pre_logits) and _Cosine
    (per-scene and shared prototypes) on inputs and upstream gradients that are not contiguous"""
    from ao_amd.ptv2.cac import _Cosine, _WeightedSum

    case = _scene(name)
    t = C.inputs(case, tier)
    off, k, rows = _cuda(t["offset"]), t["k"], t["max_rows"]
    dout = _cuda(t["dout_sets"].transpose(0, 2, 1).copy()).transpose(1, 2)            # (b, K, C) values, strided
    for detach in (False, True):
        x, logits = _cuda(t["x"], True, strided=True), _cuda(t["logits"], not detach, strided=True)
        z, out = _WeightedSum.apply(x, logits, None, off, k, rows, t["thr"], C.PROTO_EPS, 0)
        _api((WSF, name, tier), dict(z=z, out=out), C.reference(case, tier, WSF, mode=0))
        grads = torch.autograd.grad(out, (x,) if detach else (x, logits), dout)
        ref = C.reference(case, tier, WSB, mode=0)
        _api((WSB, name, tier, "detach%d" % detach), dict(zip(("gx", "glogits"), grads)), ref)
    x = _cuda(t["x"], True, strided=True)
    z, out = _WeightedSum.apply(x, None, _cuda(t["label"]), off, k, rows, 0.0, C.MEAN_EPS, 1)
    _api((WSF, name, tier, "mode1"), dict(z=z, out=out), C.reference(case, tier, WSF, mode=1))
    (gx,) = torch.autograd.grad(out, x, dout[:1])
    _api((WSB, name, tier, "mode1"), dict(gx=gx), C.reference(case, tier, WSB, mode=1))
    for per_scene in (1, 0):
        v = C.view(case, tier, COF, per_scene=per_scene)
        x, q = _cuda(t["x"], True, strided=True), _cuda(v["q"], True)
        out = _Cosine.apply(x, q, off, rows, C.COS_SCALE)
        _api((COF, name, tier, "p%d" % per_scene), dict(out=out), C.reference(case, tier, COF, per_scene=per_scene))
        gx, gq = torch.autograd.grad(out, (x, q), _cuda(v["dout"], strided=True))
        _api((COB, name, tier, "p%d" % per_scene), dict(gx=gx, gq=gq), C.reference(case, tier, COB, per_scene=per_scene))
    assert {WSF, WSB, COF, COB} <= set(spy.names), spy.names


@pytest.mark.parametrize("name", ["k20-n257-ign30", "k65-n255-absent", "k200-n257-ign30"])
@pytest.mark.parametrize("tier", C.TIERS)
def test_distillation_through_autograd(name, tier, spy):
    """_Distill: the loss, and the gradient for an upstream scalar g that is not 1"""
    from ao_amd.ptv2.cac import _Distill

    case = next(c for c in C.CASES["distill"] if c.name == name)
    t = C.inputs(case, tier)
    pred = _cuda(t["pred"], True, strided=True)
    loss = _Distill.apply(pred, _cuda(t["soft"], strided=True), _cuda(t["label"]))
    _api((DIF, name, tier), dict(loss=loss.reshape(1)), C.reference(case, tier, DIF))
    (gp,) = torch.autograd.grad(loss, pred, torch.tensor(t["g"], dtype=torch.float32, device="cuda"))
    _api((DIB, name, tier), dict(gpred=gp), C.reference(case, tier, DIB))
    assert {DIF, DIB} <= set(spy.names), spy.names


@pytest.mark.parametrize("name", ["c13-n257-ig0.1-ii255", "c64-n257-ig0.1-ii-1", "c2-n257-ig0.1-ii-1"])
@pytest.mark.parametrize("tier", C.TIERS)
def test_cross_entropy_through_autograd(name, tier, spy):
    from ao_amd.ptv2.segmentor import cross_entropy

    case = next(c for c in C.CASES["ce"] if c.name == name)
    t = C.inputs(case, tier)
    logits = _cuda(t["logits"], True, strided=True)
    loss = cross_entropy(logits, _cuda(t["label"]), t["ignore_index"])
    _api((CEF, name, tier), dict(loss=loss.reshape(1)), C.reference(case, tier, CEF))
    (gl,) = torch.autograd.grad(loss, logits, torch.tensor(t["g"], dtype=torch.float32, device="cuda"))
    _api((CEB, name, tier), dict(g_logits=gl), C.reference(case, tier, CEB))
    assert {CEF, CEB} <= set(spy.names), spy.names


# ---------------------------------------------------------------------------------------------------------------------- coverage
def test_every_cac_and_loss_launcher_is_called_directly():
    """a tour over one case of every launcher, then the names called against the eight of the two kernel files and their two size functions (the header
    declares each of them); the worst err / bound seen in this process is printed per output, for the record"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ptv2_hip.h")) as f:
        header = f.read()
    CALLED.clear()
    for launcher in R.CONTRACTS:
        check(launcher, C.CASES[C.FAMILY[launcher]][3], "plain")
    want = set(R.CONTRACTS)
    assert len(want) == 8 and all("int %s(" % name in header for name in want)
    assert CALLED == want | {"cac_workspace_bytes", "cross_entropy_workspace_bytes"}, (sorted(want - CALLED), sorted(CALLED - want))
    for (launcher, key), (ratio, where) in sorted(WORST.items()):
        print("cac-worst %s %s %.4f %s" % (launcher, key, ratio, where))
