"""CPU: the float64 reference of the dense row kernels (tests/dense_ref64.py) is itself pinned.

  * every statement against float64 autograd of nn.BatchNorm1d / F.linear / F.relu built from TRUE statistics, to 1e-10 (this
    ties the closed-form backward with mean / rstd as operands to torch's definition);
  * the records merge (parallel-variance identity) against a direct float64 variance;
  * check_dyadic / check_guard over the WHOLE case list of tests/test_gpu_dense_f64.py: exactness of the dyadic operands in fp32
    in both associations, planted zeros in every column, the all-masked column, an empty guard band;
  * the python mirrors of the dispatch rules sit on the edges the case lists claim."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import dense_ref64 as R

F64 = torch.float64


def close(a, b, tol=1e-10):
    assert a.shape == b.shape
    assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _bn_inputs(n, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    return dict(x=r(n, c) * 1.5 + 0.3, gy=r(n, c), gamma=0.5 + torch.rand(c, generator=g, dtype=F64), beta=0.3 * r(c),
                rm=0.2 * r(c), rv=1.0 + torch.rand(c, generator=g, dtype=F64), res=r(n, c),
                rowscale=(torch.rand(n, generator=g) < 0.7).double() / 0.7)


@pytest.mark.parametrize("n,c", [(2, 4), (37, 8), (200, 12)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_statements_against_float64_autograd(n, c, training, relu):
    t = _bn_inputs(n, c, n + c)
    bn = nn.BatchNorm1d(c, eps=R.EPS, momentum=R.MOMENTUM).double().train(training)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"]); bn.bias.copy_(t["beta"]); bn.running_mean.copy_(t["rm"]); bn.running_var.copy_(t["rv"])
    x = t["x"].clone().requires_grad_(True)
    y = bn(x)
    y = F.relu(y) if relu else y
    gx, dgamma, dbeta = torch.autograd.grad(y, [x, bn.weight, bn.bias], t["gy"])
    st = R.bn_stats(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"])
    if training:
        mean, rstd = st["mean"], st["rstd"]
        close(bn.running_mean, st["run_mean"]); close(bn.running_var, st["run_var"])
        assert int(bn.num_batches_tracked) == 1
    else:
        mean, rstd = t["rm"], (t["rv"] + R.EPS).rsqrt()
    close(R.bn_apply(t["x"], mean, rstd, t["gamma"], t["beta"], relu), y.detach())
    close(t["x"] * st["sc"] + st["sh"], R.bn_apply(t["x"], st["mean"], st["rstd"], t["gamma"], t["beta"], 0))
    b = R.bn_backward(t["x"], t["gy"], mean, rstd, t["gamma"], t["beta"], relu, training)
    close(b["gx"], gx); close(b["dgamma"], dgamma); close(b["dbeta"], dbeta)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("drop", [False, True])
def test_block_tail_statements_against_float64_autograd(training, drop):
    n, c = 150, 8
    t = _bn_inputs(n, c, 5)
    bn = nn.BatchNorm1d(c, eps=R.EPS).double().train(training)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"]); bn.bias.copy_(t["beta"]); bn.running_mean.copy_(t["rm"]); bn.running_var.copy_(t["rv"])
    x, ident = t["x"].clone().requires_grad_(True), t["res"].clone().requires_grad_(True)
    rs = t["rowscale"] if drop else None
    y = F.relu(ident + (bn(x) * rs[:, None] if drop else bn(x)))
    gx, gi, dgamma, dbeta = torch.autograd.grad(y, [x, ident, bn.weight, bn.bias], t["gy"])
    if training:
        mean, rstd = t["x"].mean(0), (t["x"].var(0, unbiased=False) + R.EPS).rsqrt()
    else:
        mean, rstd = t["rm"], (t["rv"] + R.EPS).rsqrt()
    y_ref = R.bn_apply(t["x"], mean, rstd, t["gamma"], t["beta"], 1, residual=t["res"], rowscale=rs)
    close(y_ref, y.detach())
    b = R.bn_backward(t["x"], t["gy"], mean, rstd, t["gamma"], t["beta"], 1, training, y=y_ref, rowscale=rs)
    close(b["gx"], gx); close(b["g_residual"], gi); close(b["dgamma"], dgamma); close(b["dbeta"], dbeta)
    close(R.bn_true_pre(t["x"], t["gamma"], t["beta"], F64, t["res"], rs, None if training else (t["rm"], t["rv"])).relu(), y.detach())


def test_one_row_in_training_mode():
    """nn.BatchNorm1d refuses one row in training mode (the unbiased variance is 0 / 0); the launchers accept it and feed the
    running variance the biased variance, 0 (include/ptv2_hip.h), which is what R.bn_stats states"""
    bn = nn.BatchNorm1d(4).double().train()
    with pytest.raises(ValueError):
        bn(torch.zeros(1, 4, dtype=F64))
    t = _bn_inputs(1, 4)
    st = R.bn_stats(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"])
    close(st["run_var"], (1 - R.MOMENTUM) * t["rv"])
    close(st["rstd"], torch.full((4,), R.EPS ** -0.5, dtype=F64))


@pytest.mark.parametrize("kmajor", [0, 1])
def test_linear_statements_against_float64_autograd(kmajor):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    m, n, k = 70, 12, 8
    X, W = [r(m, k) for _ in range(3)], [r(k, n) if kmajor else r(n, k) for _ in range(3)]
    bias, acc, sc, sh = r(n), r(m, n), 0.5 + torch.rand(k, generator=g, dtype=F64), 0.3 * r(k)
    want = acc + sum(F.linear(F.relu(x * sc + sh), w.t() if kmajor else w) for x, w in zip(X, W)) + bias
    close(R.gemm(X, W, kmajor, bias=bias, acc=acc, xsc=sc, xsh=sh), want)
    x = X[0].clone().requires_grad_(True)
    w, b = W[1].t().contiguous().requires_grad_(True) if kmajor else W[1].clone().requires_grad_(True), bias.clone().requires_grad_(True)
    y = F.linear(F.relu(x * sc + sh), w, b)
    gy = r(m, n)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], gy)
    dW, db = R.wgrad(gy, X[0], sc, sh)
    close(dW, gw); close(db, gb)
    close(R.skinny(X[0], w.detach(), sc, sh), y.detach() - bias)
    close(gy @ w.detach() * ((X[0] * sc + sh) > 0) * sc, gx)     # (the skinny input gradient gy W, chained through the transform)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 200])
def test_records_and_their_merge(m):
    g = torch.Generator().manual_seed(m)
    y = torch.randn(m, 8, generator=g, dtype=F64) * 2 + 5
    s, sq, cnt = R.stats_records(y)
    assert s.shape == (R.nrec(m), 8) and float(cnt.sum()) == m and float(cnt[-1]) == m - 64 * (R.nrec(m) - 1)
    for b in range(R.nrec(m)):
        blk = y[64 * b: 64 * b + 64]
        close(s[b], blk.sum(0)); close(sq[b], ((blk - blk.mean(0)) ** 2).sum(0))
    mean, var = R.merge_stats(s, sq, cnt)
    close(mean, y.mean(0)); close(var, y.var(0, unbiased=False))
    t = {k: v.double() for k, v in R.dyadic_bn(m, 8, 1).items()}
    rg, rgx = R.bnbwd_records(y, t, 1, F64)
    full = R.bn_backward(t["x"], y, t["mean"], t["rstd"], t["gamma"], t["beta"], 1, 0)
    close(rg.sum(0), full["dbeta"]); close(rgx.sum(0), full["dgamma"])
    rg16, _ = R.bnbwd_records(y, t, 1, F64, rows=16)
    assert rg16.shape[0] == R.nrec(m, 16)
    close(rg16.sum(0), full["dbeta"])


def _dyadic_shapes():
    """every (rows, columns, seed, masked column) the GPU file draws dyadic operands for"""
    shapes = set()
    for c in R.GEMM_CASES:
        for i in range(3 if c.feature != "plain" else 1):
            shapes.add((c.m, c.k, 100 + i, False))
        if c.feature.startswith("bnbwd"):
            shapes.add((c.m, c.n, 200, True))
    for c in R.WGRAD_CASES:
        if c.kind == "multi":
            shapes.add((c.n, c.cin, 300, False))
    for c in R.BN_CASES:
        if c.kind in ("operands", "records16"):
            shapes.add((c.n, c.c, 400, True))
            shapes.add((c.n, c.c, 401, True))
    for c in R.SKINNY_CASES:
        shapes.add((c.n, c.cin, 600, False))
    return sorted(shapes)


def test_check_inputs_on_the_whole_case_list():
    """a case that fails is an error, not a skip"""
    zeros = 0
    shapes = _dyadic_shapes()
    for n, c, seed, masked in shapes:
        t = R.dyadic_bn(n, c, seed, masked_col=masked)
        zeros += R.check_dyadic("dyadic-n%d-c%d-s%d" % (n, c, seed), t, masked)
        if masked and c > 1:   # the all-masked column: true dgamma = dbeta = 0 with and without the Block tail
            gy = torch.ones(n, c, dtype=F64)
            ops = [t[k] for k in ("mean", "rstd", "gamma", "beta")]
            b = R.bn_backward(t["x"], gy, *ops, 1, 1)
            assert float(b["dgamma"][1]) == 0.0 and float(b["dbeta"][1]) == 0.0
            y = R.bn_apply(t["x"], *ops, 1, residual=t["res_scaled"], rowscale=t["rowscale"])
            b = R.bn_backward(t["x"], gy, *ops, 1, 1, y=y, rowscale=t["rowscale"])
            assert float(b["dgamma"][1]) == 0.0 and float(b["dbeta"][1]) == 0.0
    assert len(shapes) > 150 and zeros > 10000


def _guard_shapes():
    out = set()
    for c in R.BN_CASES:
        if c.kind == "stats":
            for residual, drop in ((False, False), (True, False), (True, True)):
                out.add((c.n, c.c, 500 + c.n + c.c, residual, drop, False))
    for kind, n, c in R.PY_CASES:
        if kind.startswith(("bn_relu", "residual")):
            out.add((n, c, 700 + n + c, kind.startswith("residual"), kind == "residual_drop", kind.endswith("eval")))
    return sorted(out)


def test_guard_band_is_empty_on_the_whole_case_list():
    shapes = _guard_shapes()
    for n, c, seed, residual, drop, stats in shapes:
        t = R.guard_bn(n, c, seed, residual=residual, drop=drop, stats=stats)
        band = R.check_guard("guard-n%d-c%d" % (n, c), t, stats)
        assert band < 0.05, (n, c, band)
    assert len(shapes) > 100


def test_dispatch_mirrors_and_case_lists():
    assert R.column_block(120000, 48) == 48 and R.column_block(129, 48) == 16 and R.column_block(17, 52) == 64
    assert R.gemm_kernel(120000, 48, 48, 0, "default") == ("direct", 48, 48, False)
    assert R.gemm_kernel(4501, 192, 192, 1, "default") == ("lds", 32, 64, True)
    assert R.gemm_kernel(17, 192, 192, 1, "default")[0] == "lds" and R.gemm_kernel(17, 192, 192, 1, "direct") == ("direct", 16, 192, True)
    assert R.wg_chunk(R.wgrad_loop_rows(96, 96), 4)[1]
    assert [R.bn_grid(n, 48) for n in R.BN_GRID_EDGE] == [63, 64, 65]
    names = [c.name for cases in (R.GEMM_CASES, R.WGRAD_CASES, R.BN_CASES, R.SKINNY_CASES) for c in cases]
    assert len(names) == len(set(names))
    ms = {c.m for c in R.GEMM_CASES if (c.n, c.k, c.feature) == (48, 48, "plain")}
    assert ms >= set(R.GEMM_M) | {120000}
    assert {c.n for c in R.SKINNY_CASES} >= set(R.SKINNY_N) and {c.cout for c in R.SKINNY_CASES} >= set(R.SKINNY_COUT)
    assert {c.cin for c in R.SKINNY_CASES} >= set(R.SKINNY_CIN)
    with open(__file__.replace("tests/test_dense_ref64_host.py", "include/ptv2_hip.h")) as f:
        assert len(R.header_launchers(f.read())) == 22
