"""GPU: the CAC-v1m1 heads on ao_amd/csrc/cac.hip -- against the reference's own output (tests/golden/cac.npz), against the
eager formulation (AO_AMD_CAC=torch) at the configs' sizes, on the edge cases, bitwise reproducibility, the absence of host
synchronisation, autocast; the headless native PT-v2m2 backbone (num_classes=0) against the python path and the CPU oracle;
and a whole ScanNet CAC-config training step."""
import faulthandler

import numpy as np
import pytest
import torch

from tests.test_cac_host import (CE, LOV, SCANNET_CAC, TERMS, Identity, build, cac_cases, check_against_fixture, rel_l2,
                                 run_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a hang ends the process with a traceback instead of holding the card"""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _heads(k, thr, detach=True, criteria=(CE, LOV), seed=0):
    from ao_amd.ptv2 import CACSegmentor

    torch.manual_seed(seed)
    seg = CACSegmentor(num_classes=k, backbone_out_channels=48, backbone=Identity(), criteria=list(criteria),
                       conf_thresh=thr, detach_pre_logits=detach)
    with torch.no_grad():
        seg.seg_head.weight.mul_(2.5)
    return seg.cuda().train()


def _batch(rows, k, seed, ignore=0.1, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    n = sum(rows)
    feat = torch.randn(n, 48, generator=g) * scale
    label = torch.randint(0, k, (n,), generator=g)
    label[torch.rand(n, generator=g) < ignore] = -1
    off = np.cumsum(rows).tolist()
    return dict(feat=feat.cuda(), segment=label.cuda(), offset=torch.tensor(off, dtype=torch.int32).cuda(), offset_host=off)


def _step(seg, data):
    state = {k: v.clone() for k, v in seg.state_dict().items()}
    feat = data["feat"].clone().requires_grad_(True)
    seg.zero_grad(set_to_none=True)
    out = seg(dict(data, feat=feat))
    out["loss"].backward()
    terms = {t: out[t].detach().clone() for t in TERMS}
    grads = [(n, p.grad.clone()) for n, p in seg.named_parameters()] + [("feat", feat.grad.clone())]
    seg.load_state_dict(state)  # (the running statistics back to where they were)
    return terms, grads


def _compare(a, b, loss_rtol=1e-4, grad_rtol=2e-3):
    (ta, ga), (tb, gb) = a, b
    for t in TERMS:
        x, y = float(ta[t]), float(tb[t])
        assert np.isfinite(x) and abs(x - y) <= loss_rtol * max(1.0, abs(y)), (t, x, y)
    for (n, x), (_, y) in zip(ga, gb):
        if float(y.abs().max()) == 0.0:
            assert float(x.abs().max()) < 1e-6, n
            continue
        assert rel_l2(x, y) < grad_rtol, (n, rel_l2(x, y))


def _both(seg, data, monkeypatch):
    runs = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("AO_AMD_CAC", mode)
        runs[mode] = _step(seg, data)
    monkeypatch.delenv("AO_AMD_CAC")
    return runs["hip"], runs["torch"]


@pytest.mark.parametrize("name", ["k20_t075_det_celov", "k200_t0_det_celov", "k20_t0_nodet_ce", "k20_t075_nodet_ce"])
def test_hip_path_matches_the_reference(golden, name):
    case = cac_cases(golden)[name]
    check_against_fixture(case, run_case(case, "cuda"), loss_rtol=1e-4, grad_rtol=2e-3)


@pytest.mark.parametrize("k,thr", [(20, 0.75), (200, 0.0)])
def test_hip_path_matches_the_eager_path_at_config_size(monkeypatch, k, thr):
    seg = _heads(k, thr)
    data = _batch([100000, 100000, 100000], k, seed=k)
    # Lovasz sorts errors: rows whose order differs between the two paths move a little of the gradient
    _compare(*_both(seg, data, monkeypatch), grad_rtol=1e-2)


def test_detach_false_sends_the_gradient_to_the_logits(monkeypatch):
    seg = _heads(20, 0.5, detach=False, criteria=(CE,))
    _compare(*_both(seg, _batch([30000, 20000], 20, seed=3), monkeypatch))


def test_edge_cases(monkeypatch):
    # a scene whose rows all fall below the threshold (tiny features: flat softmax) and a scene with no labelled row
    seg = _heads(20, 0.75, criteria=(CE,))
    data = _batch([4000, 3000, 2000], 20, seed=4)
    data["feat"][:4000] *= 1e-3
    data["segment"][7000:] = -1
    _compare(*_both(seg, data, monkeypatch))
    # one scene
    _compare(*_both(seg, _batch([5000], 20, seed=5), monkeypatch))
    # no labelled row at all: kl_loss exactly 0 (the criteria are NaN as torch's mean cross-entropy over no rows)
    data = _batch([3000, 2000], 20, seed=6)
    data["segment"][:] = -1
    terms, grads = _step(seg, data)
    assert float(terms["kl_loss"]) == 0.0
    # K outside the specialised set: the eager path, on the GPU
    seg300 = _heads(300, 0.0, criteria=(CE,))
    terms, grads = _step(seg300, _batch([3000, 2000], 300, seed=7))
    assert np.isfinite(float(terms["loss"])) and all(torch.isfinite(g).all() for _, g in grads)


def test_two_runs_are_bitwise_identical():
    seg = _heads(200, 0.0)
    data = _batch([60000, 50000], 200, seed=8)
    a, b = _step(seg, data), _step(seg, data)
    for t in TERMS:
        assert torch.equal(a[0][t], b[0][t]), t
    for (n, x), (_, y) in zip(a[1], b[1]):
        assert torch.equal(x, y), n


def test_no_host_synchronisation():
    seg = _heads(20, 0.75)
    data = _batch([50000, 40000], 20, seed=9)
    _step(seg, data)  # warm: workspaces, the Lovasz masks
    torch.cuda.synchronize()
    feat = data["feat"].clone().requires_grad_(True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = seg(dict(data, feat=feat))
        out["loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(out["loss"].detach()).item()


def test_autocast_runs_the_kernels_in_fp32():
    seg = _heads(20, 0.75)
    data = _batch([40000, 30000], 20, seed=10)
    ref = _step(seg, data)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feat = data["feat"].clone().requires_grad_(True)
        out = seg(dict(data, feat=feat))
    assert all(out[t].dtype == torch.float32 for t in TERMS)
    out["loss"].backward()
    assert torch.isfinite(feat.grad).all()
    assert abs(float(out["loss"].detach()) - float(ref[0]["loss"])) < 0.05 * float(ref[0]["loss"])


def _headless_cfg():
    from oracle import ptv2_ref as M

    return dict(M.SCANNET_CFG, num_classes=0, drop_path_rate=0.0)


def test_headless_backbone_matches_the_python_path_and_the_oracle(monkeypatch):
    import ao_amd.ptv2 as ptv2
    from ao_amd import synth
    from ao_amd.ptv2 import native_model
    from oracle import ptv2_ref as M

    cfg = _headless_cfg()
    b = synth.scene_batch([0, 1], point_max=8000, in_channels=cfg["in_channels"], num_classes=20, room=1)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    model = ptv2.PointTransformerV2(**cfg).cuda().train()
    model.load_state_dict(M.init_state(cfg, seed=11), strict=True)
    assert native_model.supported(model, data["feat"]) and native_model.runtime(model).headless
    proj = torch.randn(48, 7, generator=torch.Generator().manual_seed(1)).cuda()
    runs = {}
    for mode in ("native", "python"):
        monkeypatch.setenv("AO_AMD_MODEL", mode)
        model.load_state_dict(M.init_state(cfg, seed=11), strict=True)
        model.zero_grad(set_to_none=True)
        feat = model(data)
        assert tuple(feat.shape) == (data["feat"].shape[0], 48)
        (feat @ proj).square().mean().backward()
        runs[mode] = (feat.detach().clone(), [(n, p.grad.clone()) for n, p in model.named_parameters()])
    (fa, ga), (fb, gb) = runs["native"], runs["python"]
    assert rel_l2(fa, fb) < 1e-4
    # (parameters whose gradient is zero up to rounding -- the attention's value biases -- are held to the gradients' scale)
    scale = max(float(y.abs().max()) for _, y in gb)
    for (n, x), (_, y) in zip(ga, gb):
        assert rel_l2(x, y) < 2e-2 or float((x - y).abs().max()) < 1e-4 * scale, (n, rel_l2(x, y))
    monkeypatch.delenv("AO_AMD_MODEL")
    ref = M.RefModule(cfg, seed=11, randomize_bn=True).train()
    cpu = {k: v.cpu() for k, v in data.items()}
    rf = ref(cpu)
    assert rel_l2(fa.cpu(), rf.detach()) < 1e-4


def test_headless_backbone_graph_direct_grads_and_pipelined(monkeypatch):
    """the headless runtime under direct gradient delivery and FlatAdamW, twice (the captured graphs replayed)"""
    import ao_amd.ptv2 as ptv2
    from ao_amd import synth
    from ao_amd.ptv2.optim import FlatAdamW
    from oracle import ptv2_ref as M

    cfg = _headless_cfg()
    b = synth.scene_batch([2, 3], point_max=30000, in_channels=cfg["in_channels"], num_classes=20, room=1)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    losses = {}
    for mode in ("autograd", "direct"):
        model = ptv2.PointTransformerV2(**cfg, native_param_grads=mode).cuda().train()
        model.load_state_dict(M.init_state(cfg, seed=12), strict=True)
        opt = FlatAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        out = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = model(data).square().mean()
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        losses[mode] = out
    assert all(np.isfinite(losses["direct"]))
    assert np.allclose(losses["autograd"], losses["direct"], rtol=1e-5, atol=0), losses


def test_scannet_cac_step_matches_the_eager_heads(monkeypatch):
    """configs/scannet/semseg-cac-v1m1-2-ptv2-lovasz.py on the native model, 2 x 100 k points: the loss and every parameter
    gradient against the same step with AO_AMD_CAC=torch (tolerances of test_gpu_lovasz.py's step test)."""
    from ao_amd import synth
    from ao_amd.ptv2 import CACSegmentor, native_model, registry
    from oracle import ptv2_ref as M
    from tests.test_registry_host import Registry

    MODELS = Registry("models")
    registry.register(MODELS=MODELS)
    cfg = dict(SCANNET_CAC)
    cfg["backbone"] = dict(cfg["backbone"], drop_path_rate=0.0)
    seg = MODELS.build(cfg).cuda().train()
    assert isinstance(seg, CACSegmentor)
    bcfg = _headless_cfg()
    seg.backbone.load_state_dict(M.init_state(bcfg, seed=31), strict=True)
    b = synth.scene_batch([0, 1], point_max=100000, in_channels=9, num_classes=20, room=1)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    data["offset_host"] = b["offset"].tolist()
    assert native_model.supported(seg.backbone, data["feat"])
    state = {k: v.clone() for k, v in seg.state_dict().items()}
    runs = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("AO_AMD_CAC", mode)
        seg.load_state_dict(state)
        seg.zero_grad(set_to_none=True)
        loss = seg(data)["loss"]
        loss.backward()
        runs[mode] = (float(loss.detach()), [(n, p.grad.clone()) for n, p in seg.named_parameters() if p.grad is not None])
    (lh, gh), (lt, gt) = runs["hip"], runs["torch"]
    assert np.isfinite(lh) and abs(lh - lt) < 2e-5 * max(1.0, abs(lt)), (lh, lt)
    assert len(gh) == len(gt) > 0
    for (n, a), (_, b2) in zip(gh, gt):
        if float(b2.double().norm()) == 0.0:
            assert float(a.abs().max()) < 1e-6, n
            continue
        assert rel_l2(a, b2) < 2e-2 or float((a - b2).abs().max()) < 1e-5, (n, rel_l2(a, b2))
