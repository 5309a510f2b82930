"""GPU: the stem of Stratified Transformer (ao_amd/stratified/kpconv.py, ao_amd/csrc/kpconv.hip) against tests/st_ref.py: the ball
query with truncation exercised, exactly; KPConv forward and backward against float64 under the rule of
tests/test_gpu_st_ops.py (e_kernel <= M * max(e_eager, 2^-24), M twice the worst measured ratio as a power of two).

tests/st_ref.py restates the published definitions of tp.ball_query and KPConvLayer; neither library is available to check the
restatement itself."""
import numpy as np
import pytest
import torch

from tests import st_ref as R
from tests.test_gpu_st_ops import FLOOR, _l2, _peak

pytestmark = pytest.mark.gpu

M = {"out": 8, "g_feats": 4, "g_weight": 2}


def cloud(sizes, seed, spread):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(0, spread, (n, 3)) for n in sizes]).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.tensor(np.cumsum(sizes), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("sizes,radius,max_n", [((40,), 0.9, 6), ((150, 90), 0.5, 8), ((120, 70, 102), 0.3, 5), ((300, 1, 64), 0.6, 34)])
def test_ball_query_is_exact(sizes, radius, max_n):
    from ao_amd import stratified

    x, offset = cloud(sizes, 3, 1.5)
    batch = R.offset2batch(offset, x.shape[0])
    want = R.ball_query(radius, max_n, x, batch)
    got = stratified.ball_query(radius, max_n, x, offset)
    assert got.dtype == torch.int64 and got.shape == (x.shape[0], max_n)
    assert torch.equal(got, want)
    full = (want < x.shape[0]).sum(1)
    assert int(full.max()) == max_n and int(full.min()) >= 1            # some row is cut, every row holds its own point
    dense = ((x.unsqueeze(1) - x.unsqueeze(0)) ** 2).sum(-1) < radius * radius
    assert int((dense & (batch.view(-1, 1) == batch.view(1, -1))).sum(1).max()) > max_n   # truncation is exercised


@pytest.mark.parametrize("path", ["fused", "torch"])
@pytest.mark.parametrize("sizes,cin,cout", [((40,), 3, 8), ((150, 90), 6, 16), ((120, 70, 102), 12, 12)])
def test_kpconv_against_float64(sizes, cin, cout, path, monkeypatch):
    from ao_amd import stratified

    monkeypatch.setenv("AO_AMD_ST", path)
    x, offset = cloud(sizes, 4, 1.5)
    n = x.shape[0]
    nbr = R.ball_query(0.5, 8, x, R.offset2batch(offset, n))
    gen = torch.Generator(device="cuda").manual_seed(cin)
    feats = torch.randn((n, cin), device="cuda", generator=gen)
    weight = torch.randn((15, cin, cout), device="cuda", generator=gen) / (15 * cin) ** 0.5
    g = torch.randn((n, cout), device="cuda", generator=gen)
    extent = 0.2
    runs = []
    for dtype in (torch.float64, torch.float32):
        f, w = feats.to(dtype).requires_grad_(True), weight.to(dtype).requires_grad_(True)
        out = R.kpconv(x.to(dtype), nbr, f, w, R.kernel_points(extent, dtype).cuda(), extent)
        runs.append(dict(zip(("out", "g_feats", "g_weight"), (out.detach(),) + torch.autograd.grad(out, (f, w), g.to(dtype)))))
    layer = stratified.KPConvLayer(cin, cout, point_influence=extent).cuda()
    assert not layer.K_points.requires_grad and torch.equal(layer.K_points.cpu(), R.kernel_points(extent))
    with torch.no_grad():
        layer.weight.copy_(weight)
    f = feats.clone().requires_grad_(True)
    out = layer(x, x, nbr, f)
    res = dict(zip(("out", "g_feats", "g_weight"), (out.detach(),) + torch.autograd.grad(out, (f, layer.weight), g)))
    bad = []
    for key in ("out", "g_feats", "g_weight"):
        kinds = [("l2", _l2(res[key], runs[0][key]), _l2(runs[1][key], runs[0][key]))]
        if key == "out":
            kinds.append(("peak", _peak(res[key], runs[0][key]), _peak(runs[1][key], runs[0][key])))
        for kind, got, eager in kinds:
            print("st-ratio kpconv/%s/%d %-9s %-4s kernel %.3e  eager %.3e  ratio %.3f" % (path, cin, key, kind, got, eager, got / max(eager, FLOOR)))
            if not got <= M[key] * max(eager, FLOOR):
                bad.append((key, kind, got, eager))
    assert not bad, bad


def test_kpconv_backward_repeats_bit_for_bit(monkeypatch):
    from ao_amd import stratified

    monkeypatch.setenv("AO_AMD_ST", "fused")
    x, offset = cloud((150, 90), 4, 1.5)
    nbr = stratified.ball_query(0.5, 8, x, offset)
    feats = torch.randn((240, 6), device="cuda")
    kp = stratified.kernel_points(0.2).cuda()
    grads = []
    for _ in range(2):
        f = feats.clone().requires_grad_(True)
        out = stratified.weighted_features(x, nbr, f, kp, 0.2)
        grads.append(torch.autograd.grad(out, f, torch.ones_like(out))[0])
    assert torch.equal(grads[0], grads[1])
