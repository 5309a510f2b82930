"""Float64 reference of the dense row kernels (ao_amd/csrc/gemm.hip and ao_amd/csrc/bn.hip, wgrad.hip, skinny.hip) and inputs on
which no ReLU mask can flip.

Test infrastructure (plain torch, no project kernels).  Every statement below is written from the contracts documented in
include/ptv2_hip.h ("per-point dense layers", "fp32 row GEMM"), takes a `dtype` and is evaluated twice: in float64 (the
reference) and in fp32 on the test device (the eager statement whose own distance from float64 scales the bound of the kernels,
as tests/gva_ref64.py::statement does for the attention kernels).  tests/test_dense_ref64_host.py ties the closed-form
BatchNorm backward to float64 autograd of nn.BatchNorm1d / F.linear / F.relu.

Why special inputs.  A fp32 kernel and a float64 reference that disagree on the sign of ONE pre-activation differ by a whole
term, not by rounding.  Two constructions keep every mask bit equal:

  dyadic operands (dyadic_bn): wherever the statistics are OPERANDS of the call (bn_apply*, every bn_backward*, the xsc / xsh
    operand transform of rows_gemm_fused / linear_wgrad_multi / skinny_linear_forward_xf, the bnbwd epilogue)
        x      multiples of 2^-6, |x| <= 8            mean   multiples of 2^-6 in [-2, 2]
        rstd   multiples of 2^-2 in [0.5, 2.5]        gamma  multiples of 2^-3 in [0.5, 1.5]
        beta   = -rstd gamma d with d in {-1, -1/2, 0, 1/2, 1}: multiples of 2^-6, |beta| <= 3.75
    x - mean is a multiple of 2^-6 below 2^4 (10 bits), times rstd a multiple of 2^-8 below 2^5 (13 bits), times gamma a
    multiple of 2^-11 below 2^6 (17 bits), plus beta still a multiple of 2^-11 below 2^6.  The folded form has
    sc = rstd gamma (multiple of 2^-5, <= 3.75), sh = beta - mean sc = -sc (d + mean) (multiple of 2^-11, |sh| <= 11.25) and
    x sc + sh a multiple of 2^-11 below 2^6.  Every product and every partial sum is an integer of at most 17 bits times 2^-11:
    exact in fp32 in either association, with or without fused multiply-add (gemm.hip masks on fma(h, gamma, beta), the other
    kernels on x sc + sh).  A pre-activation is exactly 0 or at least 2^-11 away from it.  Exact zeros are planted in three rows
    of every column (x = mean + d, the last row among them: the ragged tail), ReLU'(0) = 0 on both sides.  The Block tail adds
    residual (multiples of 2^-6, |.| <= 4) + rowscale in {0, 1, 5/4} times the above: multiples of 2^-13 below 2^7 (20 bits),
    zeros planted with residual = -rowscale BN(x).  mean / rstd are NOT the statistics of x: the contract is a function of the
    operands given.  Column 1 is masked everywhere (x <= mean and d >= 0 there; residual <= 0): true dgamma = dbeta = 0.

  guard band (guard_bn): where the call computes its own statistics and a ReLU follows (bn_forward with relu / residual,
    RowBatchNorm1d / bn_residual_relu through autograd) exactness is not available.  x is adjusted until every float64
    pre-activation is at least `band` away from 0, band = 2^10 x the largest fp32-vs-float64 pre-activation difference of the
    EAGER statement on that very input.  No element is left out of a comparison.

check_dyadic / check_guard assert all of this for every case (on the CPU too: tests/test_dense_ref64_host.py runs them over the
whole case list).  Weights, upstream gradients, biases and accumulate targets are generic random."""
import collections
import math

import torch

from tests.gva_ref64 import errors  # noqa: F401  (relative L2, largest element error over largest reference element)

EPS, MOMENTUM = 1e-5, 0.1

# ---------------------------------------------------------------------------------------------------------------- dispatch rules
# python mirrors of the launchers' shape rules (gemm.hip: column_block, launch_gemm_direct, ksplit_ok; wgrad.hip: wg_chunk;
# dense_common.h: bn_grid; bn.hip: finapply_ok): the case lists below are placed on both sides of every switch with them, and the tests assert that the
# cases reach every kernel family.
BM = 64


def column_block(m, n, products=1):
    wide = 48 if n % 48 == 0 else 64
    rbs = (m + BM - 1) // BM
    if rbs * ((n + wide - 1) // wide) * products >= 768 or n % 16 != 0:
        return wide
    if n % 32 == 0 and rbs * (n // 32) * products >= 256:
        return 32
    return 16


def gemm_kernel(m, n, k, kmajor, form, products=1):
    """(family, BN, KC or K, kmajor) the launcher picks for a call under AO_AMD_GEMM = form ('default' | 'lds' | 'direct')"""
    bn = column_block(m, n, products)
    direct_inst = bn in (16, 48) and k in (48, 96, 192, 384)
    pays = k == 48 or (not kmajor and bn == 48 and k <= 192)
    if form != "lds" and direct_inst and (form == "direct" or pays):
        return ("direct", bn, k, bool(kmajor))
    return ("lds", bn, 64 if k >= 192 else 32, bool(kmajor))


def ksplit_eligible(m, n, k):
    return 1 <= m <= 32768 and k in (96, 192, 384) and n % 16 == 0 and n >= 16


def wg_chunk(n, tiles):
    """(rows per split-K workgroup, whether the 'not a multiple of 8 chunks' loop moved it)"""
    chunks = max(1, 768 // max(1, tiles))
    rows = (n + chunks - 1) // chunks
    chunk = max(256, (rows + 127) // 128 * 128)
    fired = False
    if tiles > 1:
        guard = 0
        while ((n + chunk - 1) // chunk) % 8 == 0 and (n + chunk - 1) // chunk > 1 and guard < 16:
            chunk += 128
            guard += 1
            fired = True
    return min(chunk, 1 << 20), fired


def bn_grid(n, c):
    rl = max(1, 256 // (c >> 2))
    return max(1, min((n + rl * 4 - 1) // (rl * 4), 128 if n <= 16384 else 512))


def finapply_ok(n, nrec):
    return nrec <= 640 and n <= 16384


# --------------------------------------------------------------------------------------------------------------------- case lists
GemmCase = collections.namedtuple("GemmCase", "name m n k kmajor feature")
WgradCase = collections.namedtuple("WgradCase", "name n cout cin kind count")
BnCase = collections.namedtuple("BnCase", "name n c kind")
SkinnyCase = collections.namedtuple("SkinnyCase", "name n cin cout")

GEMM_M = (1, 15, 16, 17, 63, 64, 65, 127, 129, 1074, 4501, 18905)
GEMM_FEATURES = ("multi3", "sum2acc", "sum3", "xf_stats", "xf_stats3", "sum2_stats", "bnbwd1_relu", "bnbwd2", "bnbwd3_relu")


def threshold_rows(n):
    """m just below / above column_block's 768- and 256-workgroup switches for n columns (n % 48 == 0, n % 32 == 0)"""
    wide_rbs = -(-768 // (n // 48))
    mid_rbs = -(-256 // (n // 32))
    return ((mid_rbs - 1) * BM, (mid_rbs - 1) * BM + 1, (wide_rbs - 1) * BM, (wide_rbs - 1) * BM + 1)


def _gemm_cases():
    shapes = []
    for n, k in ((48, 48), (96, 96)):
        shapes += [(m, n, k) for m in GEMM_M]
    shapes.append((120000, 48, 48))
    # every direct instance (K 48 / 96 / 192 / 384), KC 32 and 64, the model's rectangular Linears, a partial column block of
    # the 64-wide path (52, 20, 100, 516), k not a multiple of the k-chunk (4, 20, 100, 196), the k-split form's 32- and
    # 16-column instances (32 x 96, 16 x 192)
    for n, k in ((192, 192), (384, 384), (512, 512), (96, 48), (192, 96), (384, 192), (512, 384), (48, 96), (48, 192), (48, 384),
                 (52, 48), (20, 48), (100, 96), (516, 192), (48, 4), (48, 20), (48, 100), (64, 196), (32, 96), (16, 192)):
        shapes += [(m, n, k) for m in (17, 129, 1074)]
    shapes += [(4501, 192, 192), (4501, 384, 384), (18905, 192, 96), (120000, 96, 48), (120000, 48, 96)]
    for n in (96, 192, 384):
        shapes += [(m, n, n) for m in threshold_rows(n)]
    out = []
    for m, n, k in shapes:
        for kmajor in (0, 1):
            out.append(GemmCase("gemm-%sm%d-n%d-k%d-km%d" % ("ks-" if ksplit_eligible(m, n, k) else "", m, n, k, kmajor),
                                m, n, k, kmajor, "plain"))
    # the fused features on a reduced shape set: one shape per kernel family (direct 16 / 48, LDS 16 / 32 / 48 / 64, both KC)
    for m, n, k in ((129, 48, 48), (120000, 48, 48), (1074, 96, 96), (4501, 192, 192), (5441, 96, 96), (1074, 384, 384),
                    (333, 52, 100), (70, 512, 196)):
        for kmajor in (0, 1):
            for f in GEMM_FEATURES:
                out.append(GemmCase("gemm-%sm%d-n%d-k%d-km%d-%s" % ("ks-" if ksplit_eligible(m, n, k) else "", m, n, k, kmajor, f),
                                    m, n, k, kmajor, f))
    return out


GEMM_CASES = _gemm_cases()
GEMM_REFUSED = ((1000, 13, 48), (1000, 48, 6), (1000, 48, 50), (64, 0, 48))   # n % 4, k % 4 (the 6 -> 48 embedding), n < 4


def gemm_products(case):
    return 3 if case.feature in ("multi3", "xf_stats3") else 1


def gemm_forms(case):
    """the AO_AMD_GEMM settings that select distinct kernels for the case (the same kernel is not run twice)"""
    seen, forms = set(), []
    for form in ("default", "lds", "direct"):
        kern = gemm_kernel(case.m, case.n, case.k, case.kmajor, form, gemm_products(case))
        if kern not in seen:
            seen.add(kern)
            forms.append(form)
    return forms


def wgrad_loop_rows(cout, cin, batch=1):
    """an n for which wg_chunk's 'not a multiple of 8 chunks' loop fires"""
    tiles = ((cout + 47) // 48) * ((cin + 47) // 48) * batch
    for n in range(1500, 40000, 61):
        if wg_chunk(n, tiles)[1]:
            return n
    raise AssertionError("no row count reaches the loop")


WGRAD_N = (1, 127, 128, 129, 255, 256, 257, 4501, 120000)


def _wgrad_cases():
    out = []

    def add(n, cout, cin, kind="plain", count=1):
        out.append(WgradCase("wgrad-%s%d-n%d-%dx%d" % (kind, count, n, cout, cin), n, cout, cin, kind, count))

    for n in WGRAD_N + (wgrad_loop_rows(96, 96),):
        add(n, 96 if n != 120000 else 48, 96 if n != 120000 else 48)
    for n in (1, 129, 257, 4501):
        add(n, 48, 48)
        add(n, 6, 48)          # direct form (cout % 4 != 0)
        add(n, 13, 48)
        add(n, 48, 6)          # direct form (cin % 4 != 0)
        add(n, 52, 100)        # ragged against the 48 x 48 output tile
        add(n, 48, 48, "offset")   # a % 4 shape whose operands start one float off a 16-byte boundary: direct form
    add(120000, 13, 48)
    for count in (1, 2, 3, 4, 5, 6):
        for n in (257, 4501):
            add(n, 48, 48, "multi", count)
        add(1074, 24, 192, "multi", count)
    add(120000, 48, 48, "multi", 3)
    for batch, cin, n in ((1, 48, 4501), (6, 48, 4501), (6, 48, 129), (48, 384, 1074), (48, 384, 1)):
        add(n, 8, cin, "strided", batch)
    add(4501, 8, 48, "padded", 6)   # ldy > batch * cout, ldx > batch * cin
    add(257, 6, 48, "padded", 3)    # the same in the direct form (cout % 4 != 0)
    return out


WGRAD_CASES = _wgrad_cases()

BN_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1074, 4501, 16384, 16385, 18905, 120000)
BN_C = (4, 8, 48, 96, 192, 384, 512, 1024)
BN_GRID_EDGE = (63 * 84, 63 * 84 + 1, 64 * 84 + 1)      # bn_grid(n, 48) = 63 / 64 / 65 records (21 row lanes x 4 rows each)
BN_REC_EDGE = (640 * 16, 640 * 16 + 1)                  # 640 / 641 records of 16 rows: finapply_ok's record limit
BN_FOLD_N = 4096 * 64 + 1                               # 4097 records of 64 rows: bn_tiles_finalize folds in two levels


def _bn_cases():
    out, seen = [], set()

    def add(n, c, kind):
        if (n, c, kind) not in seen:
            seen.add((n, c, kind))
            out.append(BnCase("bn-%s-n%d-c%d" % (kind, n, c), n, c, kind))

    for kind in ("operands", "stats"):
        for c in (48, 192):
            for n in BN_N + BN_GRID_EDGE:
                add(n, c, kind)
        for c in BN_C:
            for n in (3, 129, 4501):
                add(n, c, kind)
    for n in (3, 129, 4501):
        add(n, 48, "const")      # stats with a constant column (var = 0, rstd = eps^-1/2)
    for n in BN_REC_EDGE:
        add(n, 48, "records16")
    add(BN_FOLD_N, 8, "fold")
    return out


BN_CASES = _bn_cases()

SKINNY_COUT = (1, 4, 6, 12, 13, 24, 48, 64)
SKINNY_CIN = (4, 48, 96, 192, 384, 512)
SKINNY_N = (1, 3, 255, 256, 257, 4501, 120000)


def _skinny_cases():
    out, seen = [], set()

    def add(n, cin, cout):
        if (n, cin, cout) not in seen:
            seen.add((n, cin, cout))
            out.append(SkinnyCase("skinny-n%d-%dto%d" % (n, cin, cout), n, cin, cout))

    for n in SKINNY_N:
        add(n, 48, 6)
    for cout in SKINNY_COUT:
        for n in (3, 257, 4501):
            add(n, 48, cout)
    for cin in SKINNY_CIN:
        for n in (1, 256, 4501):
            add(n, cin, 12)
    add(257, 512, 64)
    add(1074, 384, 48)
    return out


SKINNY_CASES = _skinny_cases()
SKINNY_BWD_WIDE = (SkinnyCase("skinny-n257-48to65", 257, 48, 65), SkinnyCase("skinny-n257-48to128", 257, 48, 128))

# (kind, n, c): the Python layer through autograd on guard-band inputs
PY_CASES = (("bn", 129, 48), ("bn", 4501, 192), ("bn_relu", 3, 48), ("bn_relu", 129, 48), ("bn_relu", 4501, 192),
            ("bn_relu", 18905, 96), ("bn_relu_eval", 4501, 192), ("residual", 129, 48), ("residual", 4501, 192),
            ("residual_drop", 4501, 192), ("residual_eval", 1074, 384), ("linear", 4501, 192), ("linear", 129, 48),
            ("linear_nobias", 18905, 96), ("skinny", 4501, 192), ("skinny", 129, 48))


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(t, step, lo, hi):
    return (torch.round(t / step) * step).clamp(lo, hi)


PLANT_D = (-1.0, -0.5, 0.0, 0.5, 1.0)


def planted_rows(n, j):
    return sorted({j % n, (j + 7) % n, n - 1})


def dyadic_bn(n, c, seed, device="cpu", masked_col=True, residual=True):
    """operands of a BatchNorm (+ ReLU) (+ Block tail) on the dyadic grids of the module docstring, fp32 on `device`"""
    g = _gen(seed)
    x = _grid(2.5 * torch.randn(n, c, generator=g), 2.0 ** -6, -8.0, 8.0)
    mean = _grid(torch.randn(c, generator=g), 2.0 ** -6, -2.0, 2.0)
    rstd = _grid(0.5 + 2.0 * torch.rand(c, generator=g), 2.0 ** -2, 0.5, 2.5)
    gamma = _grid(0.5 + torch.rand(c, generator=g), 2.0 ** -3, 0.5, 1.5)
    d = torch.tensor(PLANT_D)[torch.randint(0, 5, (c,), generator=g)]
    masked_col = masked_col and c > 1
    if masked_col:
        d[1] = d[1].abs()
        x[:, 1] = mean[1] - (x[:, 1] - mean[1]).abs().clamp(max=6.0)
    rows = torch.tensor([planted_rows(n, j) + [n - 1] * (3 - len(planted_rows(n, j))) for j in range(c)])   # (c, 3)
    cols = torch.arange(c)[:, None].expand_as(rows)
    keep = x[:, 1].clone() if masked_col else None
    x[rows, cols] = (mean + d)[:, None].expand_as(rows)
    if masked_col:
        x[:, 1] = keep
    sc = rstd * gamma
    beta = -sc * d
    sh = beta - mean * sc
    t = dict(x=x, mean=mean, rstd=rstd, gamma=gamma, beta=beta, sc=sc, sh=sh)
    if residual:
        rowscale = torch.tensor([0.0, 1.0, 1.25])[torch.randint(0, 3, (n,), generator=g)]
        rowscale[-1] = 1.25
        res = _grid(torch.randn(n, c, generator=g), 2.0 ** -6, -4.0, 4.0)
        bn = (x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
        for name, rs in (("res_plain", torch.ones(n)), ("res_scaled", rowscale)):
            r = res.clone()
            if masked_col:
                r[:, 1] = -r[:, 1].abs()
            r[rows, cols] = (-rs.double()[rows] * bn[rows, cols]).float()
            t[name] = r
        t["rowscale"] = rowscale
    return {k: v.to(device).contiguous() for k, v in t.items()}


def bn_pre(t, dtype, form):
    """the BatchNorm output before the ReLU in `dtype`: 'chain' ((x - mean) rstd) gamma + beta or 'folded' x sc + sh"""
    x = t["x"].to(dtype)
    if form == "folded":
        return x * t["sc"].to(dtype) + t["sh"].to(dtype)
    return (x - t["mean"].to(dtype)) * t["rstd"].to(dtype) * t["gamma"].to(dtype) + t["beta"].to(dtype)


def _fp32_exact(v64):
    return torch.equal(v64.float().double(), v64)


def check_dyadic(name, t, masked_col=True):
    """the properties the comparison rests on; returns the number of exact zeros"""
    for key, step, lo, hi in (("x", 2.0 ** -6, -8.0, 8.0), ("mean", 2.0 ** -6, -2.0, 2.0), ("rstd", 2.0 ** -2, 0.5, 2.5),
                              ("gamma", 2.0 ** -3, 0.5, 1.5), ("beta", 2.0 ** -6, -3.75, 3.75), ("sc", 2.0 ** -5, 0.25, 3.75),
                              ("sh", 2.0 ** -11, -11.25, 11.25)):
        v = t[key].double()
        assert torch.equal(torch.round(v / step) * step, v), (name, key, "not on its grid")
        assert float(v.min()) >= lo and float(v.max()) <= hi, (name, key, float(v.min()), float(v.max()))
    x, mean, rstd, gamma, beta, sc, sh = (t[k].double() for k in ("x", "mean", "rstd", "gamma", "beta", "sc", "sh"))
    assert torch.equal(rstd * gamma, sc) and torch.equal(beta - mean * sc, sh)
    p64 = bn_pre(t, torch.float64, "chain")
    # every intermediate of either form is a fp32 number: a fused multiply-add (one rounding of an exact value) changes nothing
    for inter in (x - mean, (x - mean) * rstd, (x - mean) * rstd * gamma, x * sc, mean * sc, p64):
        assert _fp32_exact(inter), (name, "an intermediate is not exact in fp32")
    x32, m32, r32, g32, b32 = (t[k].float() for k in ("x", "mean", "rstd", "gamma", "beta"))
    for p32 in (bn_pre(t, torch.float32, "chain"), bn_pre(t, torch.float32, "folded"), (x32 - m32) * (r32 * g32) + b32):
        assert torch.equal(p32.double(), p64), (name, "fp32 and float64 pre-activations differ")
    assert torch.equal(bn_pre(t, torch.float64, "folded"), p64)
    nz = p64[p64 != 0]
    assert nz.numel() == 0 or float(nz.abs().min()) >= 2.0 ** -11
    zeros = (p64 == 0).sum(0)
    c = p64.shape[1]
    masked_col = masked_col and c > 1
    live = [j for j in range(c) if not (masked_col and j == 1)]
    assert int(zeros[live].min()) >= 1, (name, "a column without an exact zero at the kink")
    if masked_col:
        assert float(p64[:, 1].max()) <= 0.0, (name, "column 1 is not masked everywhere")
    total = int(zeros.sum())
    if "rowscale" in t:
        rs = t["rowscale"].double()
        assert bool(((rs == 0) | (rs == 1) | (rs == 1.25)).all())
        for key, scale in (("res_plain", torch.ones_like(rs)), ("res_scaled", rs)):
            r = t[key].double()
            assert _fp32_exact(scale[:, None] * p64) and float(r.abs().max()) <= 64.0
            y64 = r + scale[:, None] * p64
            y32 = t[key].float() + scale.float()[:, None] * bn_pre(t, torch.float32, "chain")
            y32b = scale.float()[:, None] * bn_pre(t, torch.float32, "folded") + t[key].float()
            assert torch.equal(y32.double(), y64) and torch.equal(y32b.double(), y64), (name, key, "tail not exact in fp32")
            assert int((y64 == 0).sum(0).min()) >= 1, (name, key, "a column without an exact zero at the tail's kink")
            if masked_col:
                assert float(y64[:, 1].max()) <= 0.0
    return total


def bn_true_pre(x, gamma, beta, dtype, residual=None, rowscale=None, stats=None):
    """pre-activation of [ReLU](BN(x)) / ReLU(residual + rowscale BN(x)) from batch statistics (or `stats` = (mean, var))"""
    x = x.to(dtype)
    mean, var = (x.mean(0), x.var(0, unbiased=False)) if stats is None else (stats[0].to(dtype), stats[1].to(dtype))
    y = (x - mean) * (var + EPS).rsqrt() * gamma.to(dtype) + beta.to(dtype)
    if residual is not None:
        y = residual.to(dtype) + (y if rowscale is None else rowscale.to(dtype)[:, None] * y)
    return y


def guard_measure(t, stats=False):
    """(band, mask of the elements inside it, float64 pre-activation) of the inputs t"""
    st = (t["rm"], t["rv"]) if stats else None
    p64 = bn_true_pre(t["x"], t["gamma"], t["beta"], torch.float64, t.get("res"), t.get("rowscale"), st)
    p32 = bn_true_pre(t["x"], t["gamma"], t["beta"], torch.float32, t.get("res"), t.get("rowscale"), st)
    band = 2.0 ** 10 * float((p32.double() - p64).abs().max())
    return band, p64.abs() < band, p64


def guard_bn(n, c, seed, device="cpu", residual=False, drop=False, stats=False):
    """generic BatchNorm inputs whose float64 pre-activations keep a guard band around 0 (module docstring).  stats: the
    pre-activation is taken from the running statistics rm / rv (eval mode).  With DropPath the rows whose rowscale is 0 have
    pre-activation = residual, which x cannot move: there the residual itself is pushed."""
    g = _gen(seed)
    t = dict(x=(torch.randn(n, c, generator=g) * 1.5 + 0.3), gamma=0.5 + torch.rand(c, generator=g),
             beta=0.3 * torch.randn(c, generator=g), rm=0.3 + 0.2 * torch.randn(c, generator=g),
             rv=1.5 + 1.5 * torch.rand(c, generator=g), gy=torch.randn(n, c, generator=g))
    if residual:
        t["res"] = torch.randn(n, c, generator=g)
    if drop:
        t["rowscale"] = (torch.rand(n, generator=g) < 0.7).float() / 0.7
    t = {k: v.to(device).contiguous() for k, v in t.items()}
    for _ in range(12):
        band, inside, p64 = guard_measure(t, stats)
        if int(inside.sum()) == 0:
            return t
        sign = torch.where(p64 >= 0, 1.0, -1.0).double()
        if "res" in t:   # the residual enters the pre-activation with weight 1: 16 bands' worth in the direction it leans
            t["res"] = torch.where(inside, t["res"].double() + sign * 16.0 * band, t["res"].double()).float().contiguous()
        else:
            var = t["rv"].double() if stats else t["x"].double().var(0, unbiased=False)
            step = (16.0 * band / (t["gamma"].double() * (var + EPS).rsqrt()))[None, :]
            t["x"] = torch.where(inside, t["x"].double() + sign * step, t["x"].double()).float().contiguous()
    raise AssertionError("guard band did not converge")


def check_guard(name, t, stats=False):
    band, inside, p64 = guard_measure(t, stats)
    assert int(inside.sum()) == 0, (name, int(inside.sum()), "elements inside the guard band")
    assert float(p64.abs().min()) >= band
    return band


# ------------------------------------------------------------------------------------------------------------------- statements
def gemm(X, W, kmajor, bias=None, acc=None, xsc=None, xsh=None, dtype=torch.float64):
    """Y = [acc +] sum_i f(X[i]) op(W[i]) [+ bias], f = ReLU(x xsc + xsh) when given; op(W) = W (k,n) if kmajor else W^T"""
    y = None
    for x, w in zip(X, W):
        x, w = x.to(dtype), w.to(dtype)
        if xsc is not None:
            x = torch.relu(x * xsc.to(dtype) + xsh.to(dtype))
        p = x @ (w if kmajor else w.t())
        y = p if y is None else y + p
    if bias is not None:
        y = y + bias.to(dtype)
    if acc is not None:
        y = acc.to(dtype) + y
    return y


def block_sums(v, rows=64):
    """(nrb, n) column sums of every `rows`-row block of v and the blocks' row counts (nrb, 1)"""
    m, n = v.shape
    nrb = (m + rows - 1) // rows
    pad = torch.zeros(nrb * rows - m, n, dtype=v.dtype, device=v.device)
    cnt = torch.full((nrb, 1), float(rows), dtype=v.dtype, device=v.device)
    cnt[-1, 0] = m - (nrb - 1) * rows
    return torch.cat([v, pad]).view(nrb, rows, n).sum(1), cnt


def stats_records(y, rows=64):
    """the `stats` records of rows_gemm_fused: per block the column sum and the sum of squares about the block mean"""
    m, n = y.shape
    s, cnt = block_sums(y, rows)
    centred = y - (s / cnt).repeat_interleave(rows, 0)[:m]
    m2, _ = block_sums(centred * centred, rows)
    return s, m2, cnt


def merge_stats(s, m2, cnt):
    """float64 merge with the parallel-variance identity: mean and biased variance of all rows"""
    s, m2, cnt = s.double(), m2.double(), cnt.double()
    n = cnt.sum()
    total = s.sum(0)
    big = (m2 + s * s / cnt).sum(0) - total * total / n
    return total / n, (big / n).clamp_min(0.0)


def bnbwd_records(y, bn, relu, dtype, rows=64):
    """the records of rows_gemm_bnbwd: per block column sums of g' and g' xhat (g' = y masked by the ReLU of BN(bn_x))"""
    h = (bn["x"].to(dtype) - bn["mean"].to(dtype)) * bn["rstd"].to(dtype)
    d = y.to(dtype)
    if relu:
        d = d * (h * bn["gamma"].to(dtype) + bn["beta"].to(dtype) > 0)
    return block_sums(d, rows)[0], block_sums(d * h, rows)[0]


def wgrad(gy, x, xsc=None, xsh=None, dtype=torch.float64):
    gy, x = gy.to(dtype), x.to(dtype)
    if xsc is not None:
        x = torch.relu(x * xsc.to(dtype) + xsh.to(dtype))
    return gy.t() @ x, gy.sum(0)


def bn_stats(x, gamma, beta, rm, rv, dtype=torch.float64, eps=EPS, momentum=MOMENTUM):
    """batch statistics, momentum update of the running buffers (unbiased variance; n = 1: the biased one, see
    include/ptv2_hip.h) and the folded affine"""
    x = x.to(dtype)
    n = x.shape[0]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    rstd = (var + eps).rsqrt()
    unb = var * (n / (n - 1.0)) if n > 1 else var
    sc = rstd * gamma.to(dtype)
    return dict(mean=mean, rstd=rstd, run_mean=(1 - momentum) * rm.to(dtype) + momentum * mean,
                run_var=(1 - momentum) * rv.to(dtype) + momentum * unb, sc=sc, sh=beta.to(dtype) - mean * sc)


def bn_apply(x, mean, rstd, gamma, beta, relu, dtype=torch.float64, residual=None, rowscale=None):
    y = (x.to(dtype) - mean.to(dtype)) * rstd.to(dtype) * gamma.to(dtype) + beta.to(dtype)
    if residual is not None:
        return torch.relu(residual.to(dtype) + (y if rowscale is None else rowscale.to(dtype)[:, None] * y))
    return torch.relu(y) if relu else y


def bn_backward(x, gy, mean, rstd, gamma, beta, relu, training, dtype=torch.float64, y=None, rowscale=None):
    """closed form with mean / rstd as GIVEN operands.  y != None: the Block tail (mask y > 0, g_residual = gy (y > 0), the
    BatchNorm receives rowscale times it).  Returns a dict gx, dgamma, dbeta[, g_residual]"""
    x, d, mean, rstd, gamma = (v.to(dtype) for v in (x, gy, mean, rstd, gamma))
    n = x.shape[0]
    h = (x - mean) * rstd
    out = {}
    if y is not None:
        d = d * (y > 0)
        out["g_residual"] = d
        if rowscale is not None:
            d = d * rowscale.to(dtype)[:, None]
    elif relu:
        d = d * (h * gamma + beta.to(dtype) > 0)
    dbeta, dgamma = d.sum(0), (d * h).sum(0)
    gx = gamma * rstd * (d - dbeta / n - h * dgamma / n) if training else gamma * rstd * d
    out.update(gx=gx, dgamma=dgamma, dbeta=dbeta)
    return out


def skinny(x, w, xsc=None, xsh=None, dtype=torch.float64):
    x = x.to(dtype)
    if xsc is not None:
        x = torch.relu(x * xsc.to(dtype) + xsh.to(dtype))
    return x @ w.to(dtype).t()


def header_launchers(text):
    """names of the entry points declared in the sections 'per-point dense layers' and 'fp32 row GEMM' of include/ptv2_hip.h"""
    import re

    a = text.index("per-point dense layers --")
    b = text.index("whole Block, one call --")
    return set(re.findall(r"^(?:int|size_t)\s+(\w+)\s*\(", text[a:b], flags=re.M))


def nrec(m, rows=64):
    return int(math.ceil(m / rows))
