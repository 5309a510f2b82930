"""GPU: every form of the dense row kernels (ao_amd/csrc/gemm.hip and ao_amd/csrc/bn.hip, wgrad.hip, skinny.hip) against float64.

Reference: tests/dense_ref64.py -- float64 statements of the contracts in include/ptv2_hip.h, on inputs whose ReLU masks cannot
differ between fp32 and float64 (dyadic operands with exact zeros planted at the kink where the statistics are operands; a guard
band of 2^10 x the eager statement's own pre-activation error where the call computes its statistics; asserted per case).  The
bound is relative to the eager fp32 statement's OWN distance from float64 on the same inputs and device:

    e_kernel = |kernel - f64| / |f64|   <=   M[output] * e_eager,    e_eager = |statement_fp32 - f64| / |f64|

in relative L2 and in the largest element error over the largest reference element.  Outputs that the dyadic inputs make exact
in fp32 (bn_apply, bn_apply_residual, g_residual) have e_eager = 0: the kernels must be exact there too.  The planted all-masked
column's dgamma / dbeta (true value 0) are bounded by M x the eager statement's absolute noise, which is 0.  M is per output
class, twice the worst ratio measured on the MI355X rounded up to a power of two (DESIGN.md 3.4 "Parity against float64: dense
kernels" holds the table).  The compared keys of every (case, form) are asserted against an explicit list; every output buffer
is pre-filled with NaN; workspaces and record buffers are sized exactly and followed by a sentinel region that must stay
untouched.

Trimmed, with the reason: a form that selects the SAME kernel as one already run for the case is not run again (AO_AMD_GEMM=lds
/ direct where the launcher's own choice is that kernel; AO_AMD_BN_FINAPPLY=0 where finapply_ok declines anyway).  The statistics
epilogue is not crossed with accumulate != 0: include/ptv2_hip.h defines the records as statistics of Y[i] and no caller
combines them.  The fused GEMM features run on one shape per kernel family, the plain product on the full shape list."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import dense_ref64 as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64

# M per output class: 2 x the worst e_kernel / e_eager over every case and form, rounded up to a power of two
M = dict(Y=16, Yacc=8, stat_sum=8, stat_sq=8, stat_mean=4, stat_var=8, rec_g=8, rec_gx=8, sum_g=8, sum_gx=8,
         dW=4, db=8, y_xf=8, gW=2, gb=4,
         mean=64, rstd=64, run_mean=16, run_var=16, sc=32, sh=64, y=32, gx=16, dgamma=16, dbeta=32,
         g_residual=1, dgamma_masked=1, dbeta_masked=1)   # (the last three are exact: 0 <= M x 0)

CALLED = set()


def _lib():
    from ao_amd import _lib as lib
    import ao_amd.ptv2.block  # noqa: F401  (registers the rows_gemm_* signatures)

    return lib


def _call(name, *args, expect=0):
    lib = _lib()
    rc = getattr(lib.lib(), name)(*args)
    CALLED.add(name)
    assert rc == expect, (name, "returned", rc, "expected", expect)


def _size(name, *args):
    CALLED.add(name)
    return int(getattr(_lib().lib(), name)(*args))


def _st():
    return _lib().stream_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _arr(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _p(t):
    return 0 if t is None else t.data_ptr()


SENTINEL = 0xA5


def _ws(nbytes):
    """a workspace of exactly nbytes followed by a sentinel region inside the same allocation"""
    return torch.full((nbytes + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")


def _ws_intact(buf, nbytes):
    assert bool((buf[nbytes:] == SENTINEL).all()), "the bytes behind the workspace were written"


def _records(floats):
    buf = torch.full((floats + 64,), float("nan"), device="cuda")
    buf[floats:] = 12345.0
    return buf


def _records_intact(buf, floats):
    assert bool((buf[floats:] == 12345.0).all()), "the floats behind the record buffer were written"


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).cuda()


def _where(diff, ref):
    """index of the worst element and its (64-row block, 16-column block)"""
    flat = int(diff.abs().argmax())
    if diff.dim() == 2:
        r, c = divmod(flat, diff.shape[1])
        return "worst element (%d, %d): row block %d, column block %d, got - ref %.3e, ref %.3e" % (
            r, c, r // 64, c // 16, float(diff[r, c]), float(ref[r, c]))
    return "worst element %d: got - ref %.3e, ref %.3e" % (flat, float(diff.flatten()[flat]), float(ref.flatten()[flat]))


def _cls(key):
    return key.rstrip("0123456789")


def compare(name, form, got, ref, eager, expected, zero_keys=()):
    """print every figure, then hold every output to M x the eager statement's error"""
    assert set(got) == set(expected), (name, form, sorted(got), sorted(expected))
    rows = []
    for key in sorted(got):
        g, r, e = got[key].double(), ref[key].double(), eager[key].double()
        assert g.shape == r.shape, (name, form, key, g.shape, r.shape)
        finite = bool(torch.isfinite(g).all())
        if key in zero_keys:
            ek = mk = float(g.abs().max())
            ee = me = float(e.abs().max())
        else:
            ek, mk = R.errors(g, r)
            ee, me = R.errors(e, r)
        rows.append((key, ek, ee, mk, me, finite))
        print("f64d %s %s %s e_kernel %.3e e_eager %.3e ratio %.2f | max %.3e %.3e ratio %.2f" % (
            name, form, key, ek, ee, ek / max(ee, 1e-300) if ek else 0.0, mk, me, mk / max(me, 1e-300) if mk else 0.0))
    for key, ek, ee, mk, me, finite in rows:
        m = M[_cls(key)]
        where = _where(got[key].double() - ref[key].double(), ref[key].double()) if finite else ""
        assert finite, (name, form, key, "not finite (an unwritten element shows as NaN)")
        assert ek <= m * ee, (name, form, key, "relative L2", ek, ee, ek / max(ee, 1e-300), m, where)
        assert mk <= m * me, (name, form, key, "largest element", mk, me, mk / max(me, 1e-300), m, where)


_CACHE = {}


def cached(key, make):
    """inputs / references of a case, computed once (the forms of a case run back to back)"""
    if key not in _CACHE:
        value = make()
        while len(_CACHE) >= 12:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = value
    return _CACHE[key]


def dyadic(n, c, seed, masked_col=True):
    def make():
        t = R.dyadic_bn(n, c, seed, masked_col=masked_col)
        R.check_dyadic("dyadic-n%d-c%d-s%d" % (n, c, seed), t, masked_col)
        return {k: v.cuda() for k, v in t.items()}

    return cached(("dyadic", n, c, seed, masked_col), make)


# ------------------------------------------------------------------------------------------------------------------- row GEMM
def gemm_inputs(case):
    def make():
        m, n, k = case.m, case.n, case.k
        gen = torch.Generator().manual_seed(7 + m + 3 * n + 5 * k + case.kmajor)
        xs = [dyadic(m, k, 100 + i, masked_col=False) for i in range(3 if case.feature != "plain" else 1)]
        t = dict(X=[d["x"] for d in xs], xsc=xs[0]["sc"], xsh=xs[0]["sh"],
                 W=[_rand(gen, *((k, n) if case.kmajor else (n, k)), scale=k ** -0.5) for _ in range(3)],
                 bias=[_rand(gen, n) for _ in range(3)], acc=_rand(gen, m, n))
        if case.feature.startswith("bnbwd"):
            t["bn"] = dyadic(m, n, 200)
        return t

    return cached(("gemm-in", case.name), make)


def gemm_statement(case, t, dtype):
    """dict of every output of the case's feature, evaluated in dtype"""
    f, km = case.feature, case.kmajor
    X, W, b = t["X"], t["W"], t["bias"]
    out = {}

    def with_stats(tag, y):
        s, sq, cnt = R.stats_records(y)
        mean, var = R.merge_stats(s, sq, cnt)
        out.update({"stat_sum" + tag: s, "stat_sq" + tag: sq, "stat_mean" + tag: mean, "stat_var" + tag: var})

    if f == "plain":
        out["Y"] = R.gemm(X[:1], W[:1], km, bias=b[0], dtype=dtype)
        out["Yacc"] = R.gemm(X[:1], W[:1], km, acc=t["acc"], dtype=dtype)
    elif f == "multi3":
        for i, bias in enumerate((b[0], None, b[2])):
            out["Y%d" % i] = R.gemm([X[i]], [W[i]], km, bias=bias, dtype=dtype)
    elif f == "sum2acc":
        out["Y0"] = R.gemm(X[:2], W[:2], km, bias=b[0], acc=t["acc"], dtype=dtype)
    elif f == "sum3":
        out["Y0"] = R.gemm(X, W, km, dtype=dtype)
    elif f == "xf_stats":
        out["Y0"] = R.gemm(X[:1], W[:1], km, bias=b[0], xsc=t["xsc"], xsh=t["xsh"], dtype=dtype)
        with_stats("0", out["Y0"])
    elif f == "xf_stats3":
        for i, bias in enumerate((None, b[1], b[2])):
            out["Y%d" % i] = R.gemm([X[i]], [W[i]], km, bias=bias, xsc=t["xsc"], xsh=t["xsh"], dtype=dtype)
        with_stats("0", out["Y0"])
        with_stats("2", out["Y2"])
    elif f == "sum2_stats":
        out["Y0"] = R.gemm(X[:2], W[:2], km, bias=b[0], dtype=dtype)
        with_stats("0", out["Y0"])
    else:
        count, relu = int(f[5]), f.endswith("relu")
        out["Y0"] = R.gemm(X[:count], W[:count], km, dtype=dtype)
        g, gx = R.bnbwd_records(out["Y0"], t["bn"], relu, dtype)
        out.update(rec_g=g, rec_gx=gx, sum_g=g.double().sum(0), sum_gx=gx.double().sum(0))
    return out


def gemm_run(case, t):
    """the same outputs from the launchers"""
    m, n, k, km, f = case.m, case.n, case.k, case.kmajor, case.feature
    X, W, b = t["X"], t["W"], t["bias"]
    nrb = R.nrec(m)
    out, recs = {}, {}

    def stats_out(tag, buf):
        v = buf[: nrb * 2 * n].view(nrb, 2, n)
        cnt = torch.full((nrb, 1), 64.0, device="cuda", dtype=F64)
        cnt[-1, 0] = m - (nrb - 1) * 64
        mean, var = R.merge_stats(v[:, 0], v[:, 1], cnt)
        out.update({"stat_sum" + tag: v[:, 0], "stat_sq" + tag: v[:, 1], "stat_mean" + tag: mean, "stat_var" + tag: var})

    if f == "plain":
        out["Y"] = _nan(m, n)
        _call("rows_gemm_hip_launcher", m, n, k, _p(X[0]), _p(W[0]), km, _p(b[0]), _p(out["Y"]), 0, _st())
        out["Yacc"] = t["acc"].clone()
        _call("rows_gemm_hip_launcher", m, n, k, _p(X[0]), _p(W[0]), km, 0, _p(out["Yacc"]), 1, _st())
    elif f in ("multi3", "sum2acc", "sum3"):
        count, summed = {"multi3": (3, 0), "sum2acc": (2, 1), "sum3": (3, 1)}[f]
        bias = {"multi3": [b[0], None, b[2]], "sum2acc": [b[0], None], "sum3": None}[f]
        ys = [_nan(m, n) for _ in range(3)] if f == "multi3" else [t["acc"].clone() if f == "sum2acc" else _nan(m, n)]
        _call("rows_gemm_multi_hip_launcher", m, n, k, count, summed, _arr(X[:count]), _arr(W[:count]), km,
              _arr(bias) if bias else None, _arr(ys + [None] * (count - len(ys))), int(f == "sum2acc"), _st())
        out.update({"Y%d" % i: y for i, y in enumerate(ys)})
    elif f in ("xf_stats", "xf_stats3", "sum2_stats"):
        count, summed = {"xf_stats": (1, 0), "xf_stats3": (3, 0), "sum2_stats": (2, 1)}[f]
        bias = {"xf_stats": [b[0]], "xf_stats3": [None, b[1], b[2]], "sum2_stats": [b[0], None]}[f]
        ys = [_nan(m, n) for _ in range(3 if f == "xf_stats3" else 1)]
        recs = {tag: _records(nrb * 2 * n) for tag in (("0", "2") if f == "xf_stats3" else ("0",))}
        st = [recs.get(str(i)) for i in range(count)]
        xf = f != "sum2_stats"
        _call("rows_gemm_fused_hip_launcher", m, n, k, count, summed, _arr(X[:count]), _arr(W[:count]), km, _arr(bias),
              _arr(ys + [None] * (count - len(ys))), 0, _p(t["xsc"]) if xf else 0, _p(t["xsh"]) if xf else 0, _arr(st), _st())
        out.update({"Y%d" % i: y for i, y in enumerate(ys)})
        torch.cuda.synchronize()
        for tag, buf in recs.items():
            stats_out(tag, buf)
    else:
        count, relu, bn = int(f[5]), int(f.endswith("relu")), t["bn"]
        out["Y0"] = _nan(m, n)
        recs["b"] = _records(nrb * 2 * n)
        _call("rows_gemm_bnbwd_hip_launcher", m, n, k, count, _arr(X[:count]), _arr(W[:count]), km, _p(out["Y0"]), _p(bn["x"]),
              _p(bn["mean"]), _p(bn["rstd"]), _p(bn["gamma"]), _p(bn["beta"]), relu, _p(recs["b"]), _st())
        torch.cuda.synchronize()
        v = recs["b"][: nrb * 2 * n].view(nrb, 2, n)
        out.update(rec_g=v[:, 0], rec_gx=v[:, 1], sum_g=v[:, 0].double().sum(0), sum_gx=v[:, 1].double().sum(0))
    torch.cuda.synchronize()
    for buf in recs.values():   # every float of the documented 64-row form written (NaN otherwise), nothing behind it
        _records_intact(buf, nrb * 2 * n)
    return out


GEMM_KEYS = dict(plain=("Y", "Yacc"), multi3=("Y0", "Y1", "Y2"), sum2acc=("Y0",), sum3=("Y0",),
                 xf_stats=("Y0", "stat_sum0", "stat_sq0", "stat_mean0", "stat_var0"),
                 xf_stats3=("Y0", "Y1", "Y2", "stat_sum0", "stat_sq0", "stat_mean0", "stat_var0", "stat_sum2", "stat_sq2",
                            "stat_mean2", "stat_var2"),
                 sum2_stats=("Y0", "stat_sum0", "stat_sq0", "stat_mean0", "stat_var0"))
BNBWD_KEYS = ("Y0", "rec_g", "rec_gx", "sum_g", "sum_gx")

GEMM_PAIRS = [pytest.param(case, form, id="%s-%s" % (case.name, form)) for case in R.GEMM_CASES for form in R.gemm_forms(case)]
KSPLIT_COUNT = sum(1 for case in R.GEMM_CASES if R.ksplit_eligible(case.m, case.n, case.k))


def gemm_check(case, form):
    t = gemm_inputs(case)
    ref, eager = cached(("gemm-ref", case.name), lambda: (gemm_statement(case, t, F64), gemm_statement(case, t, F32)))
    compare(case.name, form, gemm_run(case, t), ref, eager, GEMM_KEYS.get(case.feature, BNBWD_KEYS))


@pytest.mark.parametrize("case,form", GEMM_PAIRS)
def test_gemm_against_float64(case, form, monkeypatch):
    """`form`: AO_AMD_GEMM as the launcher reads it per call.  With AO_AMD_GEMM_KSPLIT=1 in the environment (the child run of
    test_gemm_k_split_child) the 'default' form of the cases tagged ks- is the k-split kernel, except where records are asked
    for: those keep the documented 64-row form, which gemm_run asserts float by float."""
    if form != "default":
        monkeypatch.setenv("AO_AMD_GEMM", form)
    else:
        monkeypatch.delenv("AO_AMD_GEMM", raising=False)
    gemm_check(case, form)


def test_gemm_cases_reach_every_kernel_family():
    reached = {R.gemm_kernel(c.m, c.n, c.k, c.kmajor, f, R.gemm_products(c)) for c in R.GEMM_CASES for f in R.gemm_forms(c)}
    want = {("lds", bn, kc, km) for bn in (16, 32, 48, 64) for kc in (32, 64) for km in (False, True)}
    want |= {("direct", bn, k, km) for bn in (16, 48) for k in (48, 96, 192, 384) for km in (False, True)}
    assert want <= reached, sorted(want - reached)
    assert KSPLIT_COUNT >= 100
    for n in (96, 192, 384):   # both sides of column_block's two switches
        lo_mid, hi_mid, lo_wide, hi_wide = R.threshold_rows(n)
        assert (R.column_block(lo_mid, n), R.column_block(hi_mid, n)) == (16, 32)
        assert (R.column_block(lo_wide, n), R.column_block(hi_wide, n)) == (32, 48)
    assert {R.column_block(17, n) for n in (52, 20, 100, 516)} == {64}


def test_gemm_refusals():
    """n % 4 != 0 (the 48 -> 13 head), k % 4 != 0 (the 6 -> 48 embedding), n < 4: PTV2_ERR_ARG from every launcher"""
    one = torch.zeros(1, device="cuda")
    a = _arr([one])
    for m, n, k in R.GEMM_REFUSED:
        _call("rows_gemm_hip_launcher", m, n, k, _p(one), _p(one), 0, 0, _p(one), 0, _st(), expect=1)
        _call("rows_gemm_multi_hip_launcher", m, n, k, 1, 0, a, a, 0, None, a, 0, _st(), expect=1)
        _call("rows_gemm_fused_hip_launcher", m, n, k, 1, 0, a, a, 0, None, a, 0, 0, 0, None, _st(), expect=1)
        _call("rows_gemm_bnbwd_hip_launcher", m, n, k, 1, a, a, 0, _p(one), *([_p(one)] * 5), 0, _p(one), _st(), expect=1)
    _call("rows_gemm_multi_hip_launcher", 64, 48, 48, 4, 0, a, a, 0, None, a, 0, _st(), expect=1)                 # count > 3
    _call("rows_gemm_fused_hip_launcher", 64, 48, 48, 1, 0, a, a, 0, None, a, 0, _p(one), 0, None, _st(), expect=1)   # xsc alone


def test_gemm_k_split_child():
    """the GEMM cases the k-split kernel covers (k in {96, 192, 384}, n % 16 == 0, m <= 32768), once more in a child process with
    AO_AMD_GEMM_KSPLIT=1 (read once per process)"""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-p", "no:cacheprovider", "-k",
                        "test_gemm_against_float64 and ks- and default"], cwd=ROOT, env=dict(os.environ, AO_AMD_GEMM_KSPLIT="1"),
                       capture_output=True, text=True, timeout=900)
    print("\n".join(line[line.index("f64d "):].replace(" default ", " ksplit ") for line in r.stdout.splitlines() if "f64d " in line))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "%d passed" % KSPLIT_COUNT in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------------------------------------ weight gradients
def _offset_copy(t):
    """the same values in a buffer that starts one float behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def wgrad_check(case):
    n, cout, cin, kind, count = case.n, case.cout, case.cin, case.kind, case.count
    gen = torch.Generator().manual_seed(11 + n + 3 * cout + 5 * cin + count)
    ref, eager, got = {}, {}, {}
    if kind in ("plain", "offset"):
        gy, x = _rand(gen, n, cout), _rand(gen, n, cin)
        if kind == "offset":
            gy, x = _offset_copy(gy), _offset_copy(x)
        nbytes = _size("dense_workspace_bytes", n, cout, cin)
        ws = _ws(nbytes)
        got = dict(dW=_nan(cout, cin), db=_nan(cout))
        _call("linear_wgrad_hip_launcher", n, cout, cin, _p(gy), _p(x), _p(got["dW"]), _p(got["db"]), _p(ws), nbytes, _st())
        for res, dt in ((ref, F64), (eager, F32)):
            res["dW"], res["db"] = R.wgrad(gy, x, dtype=dt)
    elif kind == "multi":
        d = dyadic(n, cin, 300, masked_col=False)
        gys = [_rand(gen, n, cout) for _ in range(count)]
        xf = [i % 3 == 0 for i in range(count)]          # the operand transform for some products only; X shared by all
        dws = [_nan(cout, cin) for _ in range(count)]
        dbs = [None if i % 2 else _nan(cout) for i in range(count)]
        nbytes = _size("dense_workspace_bytes", n, count * cout, cin)
        ws = _ws(nbytes)
        _call("linear_wgrad_multi_hip_launcher", n, cout, cin, count, _arr(gys), _arr([d["x"]] * count), _arr(dws), _arr(dbs),
              _arr([d["sc"] if f else None for f in xf]), _arr([d["sh"] if f else None for f in xf]), _p(ws), nbytes, _st())
        for i in range(count):
            got["dW%d" % i] = dws[i]
            if dbs[i] is not None:
                got["db%d" % i] = dbs[i]
            for res, dt in ((ref, F64), (eager, F32)):
                w, b = R.wgrad(gys[i], d["x"], d["sc"] if xf[i] else None, d["sh"] if xf[i] else None, dtype=dt)
                res["dW%d" % i] = w
                if dbs[i] is not None:
                    res["db%d" % i] = b
    else:
        batch = count
        pad = 0 if kind == "strided" else (8 if cout % 4 == 0 else 3)
        ldy, ldx = batch * cout + pad, batch * cin + pad
        gy, x = _nan(n, ldy), _nan(n, ldx)              # (the padding stays NaN: a product that reads it shows)
        gy[:, : batch * cout] = _rand(gen, n, batch * cout)
        x[:, : batch * cin] = _rand(gen, n, batch * cin)
        nbytes = _size("dense_workspace_bytes", n, batch * cout, cin)
        ws = _ws(nbytes)
        got = dict(dW=_nan(batch, cout, cin), db=_nan(batch, cout))
        _call("linear_wgrad_strided_hip_launcher", n, cout, cin, batch, _p(gy), ldy, cout, _p(x), ldx, cin, _p(got["dW"]),
              _p(got["db"]), _p(ws), nbytes, _st())
        for res, dt in ((ref, F64), (eager, F32)):
            a = gy[:, : batch * cout].to(dt).view(n, batch, cout)
            b = x[:, : batch * cin].to(dt).view(n, batch, cin)
            res["dW"], res["db"] = torch.einsum("nbo,nbi->boi", a, b), a.sum(0)
    torch.cuda.synchronize()
    _ws_intact(ws, nbytes)
    compare(case.name, "default", got, ref, eager, set(ref))
    if kind == "multi":
        assert set(got) == {"dW%d" % i for i in range(count)} | {"db%d" % i for i in range(0, count, 2)}
    else:
        assert set(got) == {"dW", "db"}


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.WGRAD_CASES])
def test_wgrad_against_float64(case):
    wgrad_check(case)


def test_wgrad_cases_sit_on_the_chunk_rule():
    n = R.wgrad_loop_rows(96, 96)
    assert R.wg_chunk(n, 4)[1] and any(c.n == n and c.cout == 96 for c in R.WGRAD_CASES)
    assert {c.count for c in R.WGRAD_CASES if c.kind == "multi"} == {1, 2, 3, 4, 5, 6}
    assert {c.count for c in R.WGRAD_CASES if c.kind == "strided"} == {1, 6, 48}


# (route, batch, cout, cin, bf16 operands, weighted): the kernels linear_wgrad_strided_rowscale (ao_amd/csrc/internal.h; exported,
# not in the public header) chooses between -- the grouped projection's vector-ALU kernel (cout = 8), the LDS-staged matrix-core
# kernel with weighted bias sums, and the two that cannot form them (cin % 4 != 0: the direct fp32 kernel; bf16 operands)
ROWSCALE_ROUTES = (("grouped", 6, 8, 48, False, 1), ("lds_rs", 2, 12, 48, False, 1), ("direct", 2, 8, 6, False, 0),
                   ("bf16", 2, 12, 48, True, 0))


def _rowscale_fn():
    fn = _lib().lib().linear_wgrad_strided_rowscale
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4 + [vp, ll, ll, vp, ll, ll, vp, vp, vp, ll, ctypes.POINTER(ctypes.c_int), vp, ctypes.c_size_t, vp]
    return fn


@pytest.mark.parametrize("n", [1, 129, 1500])
@pytest.mark.parametrize("route,batch,cout,cin,bf16,weighted", ROWSCALE_ROUTES, ids=[r[0] for r in ROWSCALE_ROUTES])
def test_wgrad_rowscale_against_float64(route, batch, cout, cin, bf16, weighted, n):
    """dW[b] = gY[:, b]^T X[:, b] and the WEIGHTED bias sums db[b][o] = sum_n gY[n, b, o] rowscale[n * lds_s + b], called as the
    attention backward calls it (ldy = batch cout, ldx = batch cin, lds_s = batch).  Where the chosen kernel cannot form the
    weighted sums *weighted is 0 and db is not written at all.  bf16 operands: dW to the margins of
    tests/test_gpu_bf16.py::test_linear_wgrad_bf16_operands (5e-6 of the product of the rounded operands, 1e-2 of the fp32
    statement's float64 value)."""
    gen = torch.Generator().manual_seed(29 + n + 3 * cout + 5 * cin + batch)
    gy, x, s = _rand(gen, n, batch * cout), _rand(gen, n, batch * cin), _rand(gen, n, batch)
    nbytes = _size("dense_workspace_bytes", n, batch * cout, cin)
    ws = _ws(nbytes)
    got = dict(dW=_nan(batch, cout, cin), db=_nan(batch, cout))
    flag = ctypes.c_int(-1)
    L = _lib().lib()
    prev = L.ptv2_matmul_precision(1) if bf16 else None
    try:
        rc = _rowscale_fn()(n, cout, cin, batch, _p(gy), batch * cout, cout, _p(x), batch * cin, cin, _p(got["dW"]), _p(got["db"]),
                            _p(s), batch, ctypes.byref(flag), _p(ws), nbytes, _st())
    finally:
        if bf16:
            L.ptv2_matmul_precision(prev)
    assert rc == 0 and flag.value == weighted, (route, rc, flag.value)
    ref, eager = {}, {}
    for res, dt in ((ref, F64), (eager, F32)):
        a, b = gy.to(dt).view(n, batch, cout), x.to(dt).view(n, batch, cin)
        res["dW"], res["db"] = torch.einsum("nbo,nbi->boi", a, b), torch.einsum("nbo,nb->bo", a, s.to(dt))
    torch.cuda.synchronize()
    _ws_intact(ws, nbytes)
    if not weighted:
        assert bool(torch.isnan(got.pop("db")).all()), "db was written although *weighted is 0"
        del ref["db"], eager["db"]
    if bf16:
        rounded = torch.einsum("nbo,nbi->boi", gy.bfloat16().double().view(n, batch, cout), x.bfloat16().double().view(n, batch, cin))
        e_rounded, e_full = R.errors(got["dW"].double(), rounded)[0], R.errors(got["dW"].double(), ref["dW"])[0]
        print("f64d rowscale-%s-n%d dW: %.3e of the rounded operands' product, %.3e of the float64 statement" % (route, n, e_rounded, e_full))
        assert bool(torch.isfinite(got["dW"]).all()) and e_rounded < 5e-6 and e_full < 1e-2, (e_rounded, e_full)
        return
    compare("rowscale-%s-n%d" % (route, n), "default", got, ref, eager, set(ref))


# -------------------------------------------------------------------------------------------------------------------- BatchNorm
def _fin_forms(n, nrecs):
    return ("default", "nofin") if R.finapply_ok(n, nrecs) else ("default",)


def _bn_pairs():
    out = []
    for case in R.BN_CASES:
        if case.kind == "operands":
            groups = (("apply", None), ("backward", R.bn_grid(case.n, case.c)), ("pair", R.bn_grid(case.n, case.c)),
                      ("residual", R.bn_grid(case.n, case.c)), ("records", R.nrec(case.n)))
        elif case.kind == "records16":
            groups = (("records16", R.nrec(case.n, 16)),)
        elif case.kind == "fold":
            groups = (("tiles", None),)
        else:
            groups = (("stats", None), ("forward", None), ("tiles", None)) if case.kind == "stats" else (("stats", None),)
        for group, nrecs in groups:
            for form in (("default",) if nrecs is None else _fin_forms(case.n, nrecs)):
                out.append(pytest.param(case, group, form, id="%s-%s-%s" % (case.name, group, form)))
    return out


BWD_KEYS = ("gx", "dgamma", "dbeta")
ZERO = ("dgamma_masked", "dbeta_masked")


def _masked(res, c):
    """the all-masked column's dgamma / dbeta as outputs of their own (true value 0)"""
    if c > 1:
        res = dict(res, dgamma_masked=res["dgamma"][1:2], dbeta_masked=res["dbeta"][1:2])
    return res


def _bwd_out(n, c):
    return dict(gx=_nan(n, c), dgamma=_nan(c), dbeta=_nan(c))


def bn_operands_check(case, group, form):
    n, c = case.n, case.c
    t = dyadic(n, c, 400)
    gen = torch.Generator().manual_seed(13 + n + c)
    gy = _rand(gen, n, c)
    ops = [t[k] for k in ("mean", "rstd", "gamma", "beta")]
    tag = lambda *a: "-".join(str(v) for v in a)
    if group == "apply":
        for relu in (0, 1):
            y = _nan(n, c)
            _call("bn_apply_hip_launcher", n, c, _p(t["x"]), *map(_p, ops), relu, _p(y), _st())
            compare(case.name, tag("apply", relu), dict(y=y), dict(y=R.bn_apply(t["x"], *ops, relu)),
                    dict(y=R.bn_apply(t["x"], *ops, relu, dtype=F32)), ("y",))
        for res, rs in (("res_plain", None), ("res_scaled", t["rowscale"])):
            y = _nan(n, c)
            _call("bn_apply_residual_hip_launcher", n, c, _p(t["x"]), *map(_p, ops), _p(t[res]), _p(rs), _p(y), _st())
            compare(case.name, tag("apply", res), dict(y=y), dict(y=R.bn_apply(t["x"], *ops, 1, residual=t[res], rowscale=rs)),
                    dict(y=R.bn_apply(t["x"], *ops, 1, dtype=F32, residual=t[res], rowscale=rs)), ("y",))
        return
    nbytes = _size("dense_workspace_bytes", n, 2 * c if group == "pair" else c, c)
    ws = _ws(nbytes)
    if group == "backward":
        for relu in (0, 1):
            for training in (0, 1):
                o = _bwd_out(n, c)
                _call("bn_backward_hip_launcher", n, c, _p(t["x"]), _p(gy), *map(_p, ops), relu, training, _p(o["gx"]),
                      _p(o["dgamma"]), _p(o["dbeta"]), _p(ws), nbytes, _st())
                ref, eager = (R.bn_backward(t["x"], gy, *ops, relu, training, dtype=dt) for dt in (F64, F32))
                if relu:
                    o, ref, eager = _masked(o, c), _masked(ref, c), _masked(eager, c)
                compare(case.name, tag("backward", relu, training, form), o, ref, eager, set(ref), ZERO)
    elif group == "pair":
        t2 = dyadic(n, c, 401)
        gy2 = _rand(gen, n, c)
        ops2 = [t2[k] for k in ("mean", "rstd", "gamma", "beta")]
        for relu, training in ((1, 1), (1, 0), (0, 1)):
            o, o2 = _bwd_out(n, c), _bwd_out(n, c)
            _call("bn_backward_pair_hip_launcher", n, c, _arr([t["x"], t2["x"]]), _arr([gy, gy2]),
                  *[_arr([a, b]) for a, b in zip(ops, ops2)], relu, training, _arr([o["gx"], o2["gx"]]),
                  _arr([o["dgamma"], o2["dgamma"]]), _arr([o["dbeta"], o2["dbeta"]]), _p(ws), nbytes, _st())
            for i, (oo, tt, gg, pp) in enumerate(((o, t, gy, ops), (o2, t2, gy2, ops2))):
                ref, eager = (R.bn_backward(tt["x"], gg, *pp, relu, training, dtype=dt) for dt in (F64, F32))
                if relu:
                    oo, ref, eager = _masked(oo, c), _masked(ref, c), _masked(eager, c)
                compare(case.name, tag("pair", i, relu, training, form), oo, ref, eager, set(ref), ZERO)
    elif group == "residual":
        for res, rs in (("res_plain", None), ("res_scaled", t["rowscale"])):
            y = R.bn_apply(t["x"], *ops, 1, residual=t[res], rowscale=rs).float()   # exact in fp32 (check_dyadic)
            for training in (0, 1):
                o = dict(_bwd_out(n, c), g_residual=_nan(n, c))
                _call("bn_backward_residual_hip_launcher", n, c, _p(t["x"]), _p(gy), _p(y), _p(rs), _p(t["mean"]), _p(t["rstd"]),
                      _p(t["gamma"]), training, _p(o["gx"]), _p(o["g_residual"]), _p(o["dgamma"]), _p(o["dbeta"]), _p(ws), nbytes,
                      _st())
                ref, eager = (R.bn_backward(t["x"], gy, *ops, 1, training, dtype=dt, y=y, rowscale=rs) for dt in (F64, F32))
                compare(case.name, tag("residual", res, training, form), _masked(o, c), _masked(ref, c), _masked(eager, c),
                        set(_masked(ref, c)), ZERO)
    else:   # records: the reduce pass inside the GEMM that forms gy (k = 48, W (48, c) k-major), then bn_backward_records
        k, nrb = 48, R.nrec(n)
        xg, w = _rand(gen, n, k), _rand(gen, k, c, scale=k ** -0.5)
        for relu in (0, 1):
            gyk, rec = _nan(n, c), _records(nrb * 2 * c)
            _call("rows_gemm_bnbwd_hip_launcher", n, c, k, 1, _arr([xg]), _arr([w]), 1, _p(gyk), _p(t["x"]), *map(_p, ops), relu,
                  _p(rec), _st())
            for training in (0, 1):
                o = _bwd_out(n, c)
                _call("bn_backward_records_hip_launcher", n, c, _p(t["x"]), _p(gyk), *map(_p, ops), relu, training, _p(o["gx"]),
                      _p(o["dgamma"]), _p(o["dbeta"]), _p(rec), nrb, _st())
                ref, eager = (R.bn_backward(t["x"], R.gemm([xg], [w], 1, dtype=dt), *ops, relu, training, dtype=dt)
                              for dt in (F64, F32))
                if relu:
                    o, ref, eager = _masked(o, c), _masked(ref, c), _masked(eager, c)
                compare(case.name, tag("records", relu, training, form), o, ref, eager, set(ref), ZERO)
            torch.cuda.synchronize()
            _records_intact(rec, nrb * 2 * c)
    torch.cuda.synchronize()
    _ws_intact(ws, nbytes)


def bn_records16_check(case, form):
    """bn_backward_records on records of 16 rows each (any partition of the rows is a valid record set: the merge is a sum),
    640 and 641 of them: finapply_ok's record limit"""
    n, c = case.n, case.c
    t = dyadic(n, c, 400)
    gy = _rand(torch.Generator().manual_seed(n), n, c)
    ops = [t[k] for k in ("mean", "rstd", "gamma", "beta")]
    g, gx = R.bnbwd_records(gy, t, 1, F64, rows=16)
    rec = torch.stack([g, gx], 1).float().contiguous()
    assert rec.shape[0] in (640, 641)
    for training in (0, 1):
        o = _bwd_out(n, c)
        _call("bn_backward_records_hip_launcher", n, c, _p(t["x"]), _p(gy), *map(_p, ops), 1, training, _p(o["gx"]),
              _p(o["dgamma"]), _p(o["dbeta"]), _p(rec), rec.shape[0], _st())
        ref, eager = (_masked(R.bn_backward(t["x"], gy, *ops, 1, training, dtype=dt), c) for dt in (F64, F32))
        compare(case.name, "records16-%d-%s" % (training, form), _masked(o, c), ref, eager, set(ref), ZERO)


STATS_KEYS = ("mean", "rstd", "run_mean", "run_var")


def _stats_x(case, gen):
    x = torch.randn(case.n, case.c, generator=gen) * 1.5 + 0.3
    x[:, 0] = 100.0 + 0.5 * torch.randn(case.n, generator=gen)      # |mean| >> std: the variance must survive
    if case.kind == "const":
        x[:, 2] = 3.25                                             # var = 0: rstd = eps^-1/2
    return x.cuda()


def bn_stats_check(case, group):
    n, c = case.n, case.c
    gen = torch.Generator().manual_seed(17 + n + c)
    x = _stats_x(case, gen)
    gamma, beta = (0.5 + torch.rand(c, generator=gen)).cuda(), _rand(gen, c, scale=0.3)
    rm0, rv0 = _rand(gen, c, scale=0.3), (1.0 + torch.rand(c, generator=gen)).cuda()
    nbytes = _size("dense_workspace_bytes", n, c, c)
    ws = _ws(nbytes)

    def fresh():
        o = {k: _nan(c) for k in ("mean", "rstd", "sc", "sh")}
        o.update(run_mean=rm0.clone(), run_var=rv0.clone())
        return o, torch.full((), 41, dtype=torch.int64, device="cuda")

    if group == "stats":
        ref, eager = (R.bn_stats(x, gamma, beta, rm0, rv0, dtype=dt) for dt in (F64, F32))
        o, nbt = fresh()
        _call("bn_stats_hip_launcher", n, c, _p(x), _p(o["mean"]), _p(o["rstd"]), _p(o["run_mean"]), _p(o["run_var"]), _p(nbt),
              R.EPS, R.MOMENTUM, _p(ws), nbytes, _st())
        compare(case.name, "stats", {k: o[k] for k in STATS_KEYS}, ref, eager, STATS_KEYS)
        assert int(nbt) == 42
        if n == 1:   # include/ptv2_hip.h: the unbiased variance of one row is 0 / 0; the running variance takes the biased one (0)
            assert bool(((o["run_var"].double() - (1 - R.MOMENTUM) * rv0.double()).abs() <= 2.0 ** -22 * rv0.double()).all())
        o, nbt = fresh()
        _call("bn_stats_affine_hip_launcher", n, c, _p(x), _p(gamma), _p(beta), _p(o["mean"]), _p(o["rstd"]), _p(o["sc"]), _p(o["sh"]),
              _p(o["run_mean"]), _p(o["run_var"]), _p(nbt), R.EPS, R.MOMENTUM, _p(ws), nbytes, _st())
        compare(case.name, "stats_affine", o, ref, eager, STATS_KEYS + ("sc", "sh"))
        assert int(nbt) == 42
        o, nbt = fresh()     # running buffers NULL: statistics only, nothing tracked
        _call("bn_stats_hip_launcher", n, c, _p(x), _p(o["mean"]), _p(o["rstd"]), 0, 0, 0, R.EPS, R.MOMENTUM, _p(ws), nbytes, _st())
        compare(case.name, "stats_untracked", {k: o[k] for k in ("mean", "rstd")}, ref, eager, ("mean", "rstd"))
    elif group == "forward":
        for sub, relu, residual, drop in (("plain", 0, False, False), ("relu", 1, False, False), ("residual", 1, True, False),
                                          ("residual_drop", 1, True, True)):
            t = R.guard_bn(n, c, 500 + n + c, device="cuda", residual=residual, drop=drop)
            if relu:
                R.check_guard(case.name, t)
            ref, eager = ({**R.bn_stats(t["x"], t["gamma"], t["beta"], rm0, rv0, dtype=dt)} for dt in (F64, F32))
            for res, dt in ((ref, F64), (eager, F32)):
                pre = R.bn_true_pre(t["x"], t["gamma"], t["beta"], dt, t.get("res"), t.get("rowscale"))
                res["y"] = torch.relu(pre) if relu else pre
            o, nbt = fresh()
            o["y"] = _nan(n, c)
            _call("bn_forward_hip_launcher", n, c, _p(t["x"]), _p(t["gamma"]), _p(t["beta"]), relu, _p(o["mean"]), _p(o["rstd"]),
                  _p(o["run_mean"]), _p(o["run_var"]), _p(nbt), R.EPS, R.MOMENTUM, _p(t.get("res")), _p(t.get("rowscale")), _p(o["y"]),
                  _p(ws), nbytes, _st())
            keys = STATS_KEYS + ("y",)
            compare(case.name, "forward_" + sub, {k: o[k] for k in keys}, ref, eager, keys)
            assert int(nbt) == 42
    else:   # tiles: the statistics records of rows_gemm_fused merged by bn_tiles_finalize
        k = 48
        floats = _size("bn_tiles_floats", n, c)
        part = _records(floats)
        if case.kind == "fold":   # more than 4096 records (two-level fold): the 64-row records of x, made in float64, rounded to fp32
            s, m2, _ = R.stats_records(x.double())
            assert s.shape[0] == R.nrec(n) > 4096
            part[: s.shape[0] * 2 * c] = torch.stack([s, m2], 1).float().flatten()
            made = lambda dt: x
        else:
            xg, w, b = _rand(gen, n, k), _rand(gen, c, k, scale=k ** -0.5), _rand(gen, c, scale=3.0)
            h = _nan(n, c)
            _call("rows_gemm_fused_hip_launcher", n, c, k, 1, 0, _arr([xg]), _arr([w]), 0, _arr([b]), _arr([h]), 0, 0, 0, _arr([part]), _st())
            made = lambda dt: R.gemm([xg], [w], 0, bias=b, dtype=dt)
        o, nbt = fresh()
        _call("bn_tiles_finalize_hip_launcher", n, c, _p(part), _p(gamma), _p(beta), _p(o["mean"]), _p(o["rstd"]), _p(o["sc"]),
              _p(o["sh"]), _p(o["run_mean"]), _p(o["run_var"]), _p(nbt), R.EPS, R.MOMENTUM, _st())
        ref, eager = (R.bn_stats(made(dt), gamma, beta, rm0, rv0, dtype=dt) for dt in (F64, F32))
        compare(case.name, "tiles", o, ref, eager, STATS_KEYS + ("sc", "sh"))
        assert int(nbt) == 42
        torch.cuda.synchronize()
        _records_intact(part, floats)
    torch.cuda.synchronize()
    _ws_intact(ws, nbytes)


@pytest.mark.parametrize("case,group,form", _bn_pairs())
def test_batchnorm_against_float64(case, group, form, monkeypatch):
    """`form` nofin: AO_AMD_BN_FINAPPLY=0 (read per call), the three-launch backward where the default is finalize-in-apply"""
    if form == "nofin":
        monkeypatch.setenv("AO_AMD_BN_FINAPPLY", "0")
    else:
        monkeypatch.delenv("AO_AMD_BN_FINAPPLY", raising=False)
    if case.kind == "operands":
        bn_operands_check(case, group, form)
    elif case.kind == "records16":
        bn_records16_check(case, form)
    else:
        bn_stats_check(case, group)


def test_batchnorm_cases_sit_on_the_dispatch_edges():
    assert [R.bn_grid(n, 48) for n in R.BN_GRID_EDGE] == [63, 64, 65]
    assert [R.nrec(n, 16) for n in R.BN_REC_EDGE] == [640, 641]
    assert R.nrec(R.BN_FOLD_N) == 4097 and any(c.kind == "fold" and c.n == R.BN_FOLD_N for c in R.BN_CASES)
    assert R.finapply_ok(R.BN_REC_EDGE[0], 640) and not R.finapply_ok(R.BN_REC_EDGE[1], 641)
    assert R.finapply_ok(16384, R.bn_grid(16384, 48)) and not R.finapply_ok(16385, R.bn_grid(16385, 48))
    assert R.bn_grid(16384, 48) == 128 and R.bn_grid(120000, 48) == 512
    names = {(c.n, c.c) for c in R.BN_CASES if c.kind == "operands"}
    assert all((n, c) in names for n in R.BN_N + R.BN_GRID_EDGE for c in (48, 192))
    assert all((n, c) in names for n in (3, 129, 4501) for c in R.BN_C)


def test_batchnorm_refusals():
    one = torch.zeros(8, device="cuda")
    p = _p(one)
    _call("bn_stats_hip_launcher", 8, 6, p, p, p, 0, 0, 0, R.EPS, R.MOMENTUM, p, 1 << 20, _st(), expect=1)      # c % 4
    _call("bn_stats_hip_launcher", 8, 1028, p, p, p, 0, 0, 0, R.EPS, R.MOMENTUM, p, 1 << 20, _st(), expect=1)   # c > 1024
    _call("bn_stats_hip_launcher", 8, 8, p, p, p, 0, 0, 0, R.EPS, R.MOMENTUM, p, 16, _st(), expect=2)           # workspace
    _call("bn_backward_hip_launcher", 0, 8, p, p, p, p, p, p, 0, 0, p, p, p, p, 1 << 20, _st(), expect=1)       # n < 1
    _call("bn_apply_residual_hip_launcher", 8, 8, p, p, p, p, p, 0, 0, p, _st(), expect=1)                      # no residual


# ------------------------------------------------------------------------------------------------------------------------ skinny
def skinny_check(case, forward=True):
    n, cin, cout = case.n, case.cin, case.cout
    gen = torch.Generator().manual_seed(19 + n + cin + cout)
    w = _rand(gen, cout, cin, scale=0.2)
    got, ref, eager = {}, {}, {}
    if forward:
        x, d = _rand(gen, n, cin), dyadic(n, cin, 600, masked_col=False)
        got.update(y=_nan(n, cout), y_xf=_nan(n, cout))
        _call("skinny_linear_forward_hip_launcher", n, cin, cout, _p(x), _p(w), _p(got["y"]), _st())
        _call("skinny_linear_forward_xf_hip_launcher", n, cin, cout, _p(d["x"]), _p(w), _p(d["sc"]), _p(d["sh"]), _p(got["y_xf"]), _st())
        for res, dt in ((ref, F64), (eager, F32)):
            res.update(y=R.skinny(x, w, dtype=dt), y_xf=R.skinny(d["x"], w, d["sc"], d["sh"], dtype=dt))
    gy = _rand(gen, n, cout)
    got["gx"] = _nan(n, cin)
    _call("skinny_linear_backward_hip_launcher", n, cin, cout, _p(gy), _p(w), _p(got["gx"]), _st())
    for res, dt in ((ref, F64), (eager, F32)):
        res["gx"] = gy.to(dt) @ w.to(dt)
    torch.cuda.synchronize()
    compare(case.name, "default", got, ref, eager, ("y", "y_xf", "gx") if forward else ("gx",))


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.SKINNY_CASES])
def test_skinny_against_float64(case):
    skinny_check(case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.SKINNY_BWD_WIDE])
def test_skinny_forward_refuses_wide_outputs_and_the_backward_takes_them(case):
    """the forward keeps W in LDS and is capped at cout = 64 (PTV2_ERR_ARG beyond); the input gradient has no such cap"""
    one = torch.zeros(4, device="cuda")
    _call("skinny_linear_forward_hip_launcher", case.n, case.cin, case.cout, _p(one), _p(one), _p(one), _st(), expect=1)
    _call("skinny_linear_forward_xf_hip_launcher", case.n, case.cin, case.cout, _p(one), _p(one), 0, 0, _p(one), _st(), expect=1)
    _call("skinny_linear_forward_hip_launcher", 8, 6, 4, _p(one), _p(one), _p(one), _st(), expect=1)           # cin % 4
    skinny_check(case, forward=False)


# ------------------------------------------------------------------------------------------------------------------ python layer
def python_layer_check(kind, n, c):
    import torch.nn as nn
    import torch.nn.functional as Fn

    from ao_amd.ptv2.layers import RowBatchNorm1d, RowLinear, bn_residual_relu, skinny_linear

    name = "py-%s-n%d-c%d" % (kind, n, c)
    gen = torch.Generator().manual_seed(23 + n + c)
    if kind.startswith("linear") or kind == "skinny":
        cout = c // 8 if kind == "skinny" else (c // 2 if n % 2 else c)
        x, go = _rand(gen, n, c), _rand(gen, n, cout)
        w, b = _rand(gen, cout, c, scale=c ** -0.5), (_rand(gen, cout) if kind == "linear" else None)

        def stock(dt):
            leaves = [v.to(dt).clone().requires_grad_(True) for v in (x, w) + ((b,) if b is not None else ())]
            y = Fn.linear(*leaves)
            return dict(zip(("y", "gx", "gW", "gb"), (y.detach(),) + torch.autograd.grad(y, leaves, go.to(dt))))

        leaves = [v.clone().requires_grad_(True) for v in (x, w)]
        if kind == "skinny":
            y = skinny_linear(*leaves)
        else:
            lin = RowLinear(c, cout, bias=b is not None).cuda()
            with torch.no_grad():
                lin.weight.copy_(w)
                if b is not None:
                    lin.bias.copy_(b)
            y = lin(leaves[0])
            leaves = [leaves[0], lin.weight] + ([lin.bias] if b is not None else [])
        got = dict(zip(("y", "gx", "gW", "gb"), (y.detach(),) + torch.autograd.grad(y, leaves, go)))
        compare(name, "autograd", got, stock(F64), stock(F32), ("y", "gx", "gW") + (("gb",) if b is not None else ()))
        return
    residual, drop, evalmode = kind.startswith("residual"), kind == "residual_drop", kind.endswith("eval")
    relu = kind != "bn"
    t = R.guard_bn(n, c, 700 + n + c, device="cuda", residual=residual, drop=drop, stats=evalmode)
    if relu:
        R.check_guard(name, t, stats=evalmode)

    def stock(dt):
        bn = nn.BatchNorm1d(c, eps=R.EPS, momentum=R.MOMENTUM).cuda().to(dt).train(not evalmode)
        with torch.no_grad():
            for p, v in ((bn.weight, t["gamma"]), (bn.bias, t["beta"]), (bn.running_mean, t["rm"]), (bn.running_var, t["rv"])):
                p.copy_(v.to(dt))
        x = t["x"].to(dt).clone().requires_grad_(True)
        leaves = [x, bn.weight, bn.bias]
        y = bn(x)
        if residual:
            ident = t["res"].to(dt).clone().requires_grad_(True)
            leaves.append(ident)
            y = ident + (y * t["rowscale"].to(dt)[:, None] if drop else y)
        y = Fn.relu(y) if relu else y
        res = dict(zip(("y", "gx", "dgamma", "dbeta", "g_residual"), (y.detach(),) + torch.autograd.grad(y, leaves, t["gy"].to(dt))))
        res.update(run_mean=bn.running_mean.detach().clone(), run_var=bn.running_var.detach().clone())
        return res

    mine = RowBatchNorm1d(c, eps=R.EPS, momentum=R.MOMENTUM).cuda().train(not evalmode)
    with torch.no_grad():
        for p, v in ((mine.weight, t["gamma"]), (mine.bias, t["beta"]), (mine.running_mean, t["rm"]), (mine.running_var, t["rv"])):
            p.copy_(v)
    x = t["x"].clone().requires_grad_(True)
    leaves = [x, mine.weight, mine.bias]
    if residual:
        ident = t["res"].clone().requires_grad_(True)
        leaves.append(ident)
        y = bn_residual_relu(mine, x, ident, t["rowscale"] if drop else None)
    else:
        y = mine(x, relu)
    got = dict(zip(("y", "gx", "dgamma", "dbeta", "g_residual"), (y.detach(),) + torch.autograd.grad(y, leaves, t["gy"])))
    got.update(run_mean=mine.running_mean.detach().clone(), run_var=mine.running_var.detach().clone())
    keys = ("y", "gx", "dgamma", "dbeta", "run_mean", "run_var") + (("g_residual",) if residual else ())
    compare(name, "autograd", got, stock(F64), stock(F32), keys)


@pytest.mark.parametrize("kind,n,c", R.PY_CASES)
def test_python_layer_against_float64_autograd(kind, n, c):
    python_layer_check(kind, n, c)


# ---------------------------------------------------------------------------------------------------------------------- coverage
def test_every_dense_launcher_is_called_directly(monkeypatch):
    """every entry point of the sections 'per-point dense layers' and 'fp32 row GEMM' of include/ptv2_hip.h is called by this
    file: a tour over one small case of every runner above, then the names they called against the names the header declares"""
    monkeypatch.delenv("AO_AMD_GEMM", raising=False)
    monkeypatch.delenv("AO_AMD_BN_FINAPPLY", raising=False)
    with open(os.path.join(ROOT, "include", "ptv2_hip.h")) as f:
        declared = R.header_launchers(f.read())
    assert len(declared) == 22 and "rows_gemm_fused_hip_launcher" in declared and "bn_backward_pair_hip_launcher" in declared
    CALLED.clear()
    for feature in ("plain", "multi3", "xf_stats", "bnbwd1_relu"):
        gemm_check(next(c for c in R.GEMM_CASES if c.feature == feature), "default")
    for kind in ("plain", "multi", "strided"):
        wgrad_check(next(c for c in R.WGRAD_CASES if c.kind == kind and c.n > 1))
    case = next(c for c in R.BN_CASES if c.kind == "operands" and c.n == 129)
    for group in ("apply", "backward", "pair", "residual", "records"):
        bn_operands_check(case, group, "default")
    case = next(c for c in R.BN_CASES if c.kind == "stats" and c.n == 129)
    for group in ("stats", "forward", "tiles"):
        bn_stats_check(case, group)
    skinny_check(R.SKINNY_CASES[1])
    assert CALLED == declared, (sorted(declared - CALLED), sorted(CALLED - declared))
