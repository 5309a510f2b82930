"""GPU: the Lovasz-softmax loss on ao_amd/csrc/lovasz.hip -- against the reference's own output (tests/golden/lovasz.npz),
against an independent vectorised restatement below at the sizes of the three Lovasz configs, on exact ties (the tie rule:
equal errors in ascending row order), its edge cases, under autocast, inside a ScanNet-config training step, and without a
host synchronisation."""
import numpy as np
import pytest
import torch

from tests.test_lovasz_host import check_against_fixture, lovasz_cases

pytestmark = pytest.mark.gpu


def restatement(logits, label, ignore_index=-1, class_seen=None, weight=1.0):
    """(loss, d loss / d logits), vectorised over all classes.  p is formed in fp32 with the kernel's rounding sequence
    (m = max, s = sum over columns in order of exp(x - m), p = exp(x_c - m) / s) and the errors in fp32; the sort is torch's
    stable descending sort; g is the reference's fp32 formula; the dot products, the mean and the gradient are float64."""
    x = logits.detach().float()
    n, c = x.shape
    m = x.max(1, keepdim=True).values
    ex = torch.exp(x - m)
    s = ex[:, 0].clone()
    for j in range(1, c):
        s = s + ex[:, j]
    p = ex / s[:, None]
    used = (label != ignore_index) if ignore_index is not None else torch.ones_like(label, dtype=torch.bool)
    rows = torch.nonzero(used).flatten()
    lab = label[rows]
    fg = torch.nn.functional.one_hot(lab, c).float()
    e = (fg - p[rows]).abs()
    srt, perm = torch.sort(e, dim=0, descending=True, stable=True)
    # g in the reference's fp32 formula (lovasz.py:22-33): J_k - J_{k-1} cancels, so float64 would differ from it by up
    # to ~n ulps of J per element; the counts are exact integers in fp32
    fgs = torch.gather(fg, 0, perm)
    k = torch.arange(1, len(rows) + 1, device=x.device, dtype=torch.float32)[:, None]
    gts = fgs.sum(0)
    cum = fgs.cumsum(0)
    jac = 1.0 - (gts - cum) / (gts + (k - cum))
    g = torch.cat([jac[:1], jac[1:] - jac[:-1]], 0).double()
    keep = gts > 0
    if class_seen is not None:
        keep &= torch.isin(torch.arange(c, device=x.device), torch.tensor(class_seen, device=x.device))
    ncls = int(keep.sum())
    if ncls == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x, dtype=torch.float64)
    loss = (srt.double() * g).sum(0)[keep].sum() / ncls * weight
    g_at = torch.zeros_like(g).scatter_(0, perm, g)  # g of each row's rank, per class
    sign = torch.sign(fg - p[rows]).double()
    gp = torch.zeros(n, c, dtype=torch.float64, device=x.device)
    gp[rows] = -sign * g_at * keep.double() * (weight / ncls)
    pd = p.double()
    grad = pd * (gp - (gp * pd).sum(1, keepdim=True))
    return loss, grad


def hip_loss_and_grad(logits, label, ignore_index=-1, class_seen=None, weight=1.0):
    from ao_amd.ptv2 import lovasz_softmax

    x = logits.clone().requires_grad_(True)
    loss = lovasz_softmax(x, label, ignore_index, class_seen, weight)
    loss.backward()
    return loss.detach(), x.grad


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_hip_path_matches_the_reference(golden):
    for name, case in lovasz_cases(golden).items():
        loss, grad = hip_loss_and_grad(case["logits"].cuda(), case["label"].cuda(), case["ignore_index"], case["class_seen"],
                                       case["loss_weight"])
        check_against_fixture(case, loss.cpu(), grad.cpu())


def _scene(n, c, present, seed, ignore_frac=0.1, distinct_rows=None):
    """Random labels over `present` of the c classes and logits of a half-trained head.  distinct_rows=K: the logits rows are
    K distinct rows repeated (errors of different rows then lie far apart, equal ones tie exactly)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    classes = torch.randperm(c, generator=g, device="cuda")[:present]
    label = classes[torch.randint(0, present, (n,), generator=g, device="cuda")]
    label[torch.rand(n, generator=g, device="cuda") < ignore_frac] = -1
    if distinct_rows:
        pick = torch.randint(0, distinct_rows, (n,), generator=g, device="cuda")
        base_label = classes[torch.randint(0, present, (distinct_rows,), generator=g, device="cuda")]
        label = torch.where(label < 0, label, base_label[pick])
        base = torch.randn(distinct_rows, c, generator=g, device="cuda") * 3.0
        base[torch.arange(distinct_rows, device="cuda"), base_label] += 2.0
        return base[pick], label
    logits = torch.randn(n, c, generator=g, device="cuda") * 3.0
    logits[torch.arange(n, device="cuda"), label.clamp_min(0)] += 2.0  # a half-trained head: a spread of errors
    return logits, label


@pytest.mark.parametrize("n, c, present", [(120000, 13, 13), (200000, 20, 20), (200000, 200, 60)])
def test_hip_path_matches_the_restatement(n, c, present):
    """Random rows: the loss to 1e-6; the gradient to 2e-3 only, in case the restatement's p (torch's exp) and the kernel's
    differ in the last bit, which would reorder errors closer than that and move g between those rows.  Rows drawn from 500
    distinct rows: errors of different rows are far apart, equal ones tie exactly, and the gradient must agree to
    1e-5 -- order, ties included, is the same."""
    for distinct, tol in ((None, 2e-3), (500, 1e-5)):
        logits, label = _scene(n, c, present, seed=n + c, distinct_rows=distinct)
        loss, grad = hip_loss_and_grad(logits, label)
        rloss, rgrad = restatement(logits, label)
        assert abs(float(loss) - float(rloss)) <= 1e-6 * abs(float(rloss)), (distinct, float(loss), float(rloss))
        assert rel_l2(grad, rgrad) <= tol, (distinct, rel_l2(grad, rgrad))
        # class_seen and loss_weight on the same inputs
        seen = list(range(0, c, 3))
        loss, grad = hip_loss_and_grad(logits, label, class_seen=seen, weight=0.5)
        rloss, rgrad = restatement(logits, label, class_seen=seen, weight=0.5)
        assert abs(float(loss) - float(rloss)) <= 1e-6 * abs(float(rloss)), (distinct, float(loss), float(rloss))
        assert rel_l2(grad, rgrad) <= tol, (distinct, rel_l2(grad, rgrad))


@pytest.mark.parametrize("kind", ["duplicated_rows", "saturated"])
def test_exact_ties_follow_ascending_row_order(kind):
    g = torch.Generator(device="cuda").manual_seed(7)
    n, c = 30000, 13
    if kind == "duplicated_rows":  # 40 distinct rows, each repeated ~750 times in random order: every error ties
        base = torch.randn(40, c, generator=g, device="cuda")
        pick = torch.randint(0, 40, (n,), generator=g, device="cuda")
        logits = base[pick]
        label = torch.randint(0, c, (40,), generator=g, device="cuda")[pick]
        label[torch.rand(n, generator=g, device="cuda") < 0.2] = torch.randint(0, c, (1,), generator=g, device="cuda").item()
    else:  # saturated softmax: errors exactly 0 or 1 for most rows
        label = torch.randint(0, c, (n,), generator=g, device="cuda")
        logits = torch.randn(n, c, generator=g, device="cuda")
        sat = torch.rand(n, generator=g, device="cuda") < 0.8
        hot = torch.where(torch.rand(n, generator=g, device="cuda") < 0.7, label, (label + 1) % c)
        logits[sat] = -200.0
        logits[sat, hot[sat]] = 200.0
    label[::11] = -1
    loss, grad = hip_loss_and_grad(logits, label)
    rloss, rgrad = restatement(logits, label)
    assert abs(float(loss) - float(rloss)) <= 1e-6 * abs(float(rloss))
    # per element: a different tie order moves g between rows and shows as O(1) relative differences
    torch.testing.assert_close(grad.double(), rgrad, rtol=1e-4, atol=1e-6 * float(rgrad.abs().max()))


def test_edge_cases(monkeypatch):
    from ao_amd.ptv2 import lovasz_softmax

    logits = torch.randn(5000, 8, device="cuda")
    label = torch.randint(0, 3, (5000,), device="cuda")
    loss, grad = hip_loss_and_grad(logits, label, class_seen=[5, 6, 40])  # no class left after class_seen
    assert loss.dim() == 0 and float(loss) == 0.0 and torch.count_nonzero(grad) == 0
    loss, grad = hip_loss_and_grad(logits, torch.full_like(label, -1))  # no labelled row
    assert loss.dim() == 0 and float(loss) == 0.0 and torch.count_nonzero(grad) == 0
    bad = label.clone()
    bad[123] = 8
    assert torch.isnan(lovasz_softmax(logits, bad, -1))
    assert torch.isfinite(lovasz_softmax(logits, bad, 8))
    monkeypatch.setenv("AO_AMD_CHECK_LABELS", "1")
    with pytest.raises(ValueError):
        lovasz_softmax(logits, bad, -1)
    monkeypatch.delenv("AO_AMD_CHECK_LABELS")
    with pytest.raises(ValueError):
        lovasz_softmax(torch.randn(10, 1, device="cuda"), torch.zeros(10, dtype=torch.int64, device="cuda"), -1)
    # ignore_index=None: every row is used
    loss, grad = hip_loss_and_grad(logits, label, ignore_index=None)
    rloss, rgrad = restatement(logits, label, ignore_index=None)
    assert abs(float(loss) - float(rloss)) <= 1e-6 * float(rloss) and rel_l2(grad, rgrad) <= 1e-5
    # the same call twice: identical bits (fixed-order reductions)
    a = hip_loss_and_grad(logits, label)
    b = hip_loss_and_grad(logits, label)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_autocast_bf16_runs_in_fp32():
    from ao_amd.ptv2 import lovasz_softmax

    logits, label = _scene(60000, 20, 20, seed=3)
    w = torch.randn(20, 20, device="cuda", requires_grad=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = logits @ w  # bf16 logits
        assert h.dtype == torch.bfloat16
        loss = lovasz_softmax(h, label, -1)
    assert loss.dtype == torch.float32
    loss.backward()
    rloss, _ = restatement(h.detach().float(), label)
    assert abs(float(loss) - float(rloss)) <= 1e-6 * float(rloss)
    assert torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0


def test_no_host_synchronisation():
    from ao_amd.ptv2 import LovaszLoss

    logits, label = _scene(100000, 20, 20, seed=5)
    x = logits.clone().requires_grad_(True)
    crit = LovaszLoss("multiclass", class_seen=[0, 1, 2, 5], ignore_index=-1)
    crit(x, label).backward()  # warm: workspace, class_seen mask
    torch.cuda.synchronize()
    x.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(x, label)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss.detach()).item()


def test_scannet_step_with_ce_and_lovasz_matches_the_eager_loss(monkeypatch):
    """configs/scannet/semseg-pt-v2m2-3-lovasz.py's criteria on the native model, 2 x 100 k points: loss and every parameter
    gradient against the same step with AO_AMD_LOVASZ=torch (tolerances of test_gpu_zz_oracle_120k.py)."""
    import ao_amd.ptv2 as ptv2
    from ao_amd import synth
    from oracle import ptv2_ref as M

    cfg = dict(M.SCANNET_CFG, drop_path_rate=0.0)
    b = synth.scene_batch([0, 1], point_max=100000, in_channels=cfg["in_channels"], num_classes=cfg["num_classes"], room=1)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    criteria = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    seg = ptv2.DefaultSegmentor(dict(cfg, type="PT-v2m2"), criteria=criteria).cuda().train()
    seg.backbone.load_state_dict(M.init_state(cfg, seed=31), strict=True)
    runs = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("AO_AMD_LOVASZ", mode)
        seg.zero_grad(set_to_none=True)
        loss = seg(data)["loss"]
        loss.backward()
        runs[mode] = (float(loss.detach()), [(n, p.grad.clone()) for n, p in seg.named_parameters() if p.grad is not None])
    (lh, gh), (lt, gt) = runs["hip"], runs["torch"]
    assert np.isfinite(lh) and abs(lh - lt) < 2e-5, (lh, lt)
    assert len(gh) == len(gt) > 0
    for (n, a), (_, b2) in zip(gh, gt):
        if float(b2.double().norm()) == 0.0:
            assert float(a.abs().max()) < 1e-6, n
            continue
        assert rel_l2(a, b2) < 2e-2 or float((a - b2).abs().max()) < 1e-5, (n, rel_l2(a, b2))
