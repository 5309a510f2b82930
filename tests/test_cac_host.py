"""CPU: the CAC-v1m1 segmentor (ao_amd/ptv2/cac.py) on its eager path against the reference's own output
(tests/golden/cac.npz, tests/golden/make_golden_cac.py), its state_dict keys, its registration, construction from the two
reference CAC configs, and the criteria it refuses."""
import numpy as np
import pytest
import torch

CE = dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)
LOV = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)
TERMS = ("loss", "seg_loss", "pre_loss", "pre_self_loss", "kl_loss")

# the model dicts of configs/scannet/semseg-cac-v1m1-2-ptv2-lovasz.py and configs/scannet200/semseg-cac-v1m1-2-ptv2-lovasz.py
_PTV2_HEADLESS = dict(
    type="PT-v2m2", in_channels=9, num_classes=0, patch_embed_depth=1, patch_embed_channels=48, patch_embed_groups=6,
    patch_embed_neighbours=8, enc_depths=(2, 2, 6, 2), enc_channels=(96, 192, 384, 512), enc_groups=(12, 24, 48, 64),
    enc_neighbours=(16, 16, 16, 16), dec_depths=(1, 1, 1, 1), dec_channels=(48, 96, 192, 384), dec_groups=(6, 12, 24, 48),
    dec_neighbours=(16, 16, 16, 16), grid_sizes=(0.06, 0.15, 0.375, 0.9375), attn_qkv_bias=True, pe_multiplier=False,
    pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.3, enable_checkpoint=False, unpool_backend="map")


def cac_config(num_classes, conf_thresh):
    return dict(type="CAC-v1m1", backbone=dict(_PTV2_HEADLESS), criteria=[dict(CE), dict(LOV)], num_classes=num_classes,
                backbone_out_channels=48, cos_temp=15, main_weight=1, pre_weight=1, pre_self_weight=1, kl_weight=1,
                conf_thresh=conf_thresh, detach_pre_logits=True)


SCANNET_CAC = cac_config(20, 0.75)
SCANNET200_CAC = cac_config(200, 0)


class Identity(torch.nn.Module):
    """the fixture's backbone: returns the batch's `feat`"""

    def forward(self, data_dict):
        return data_dict["feat"]


def cac_cases(golden):
    z = golden("cac.npz")
    names = sorted({k.split("/")[0] for k in z.files if not k.startswith("param_k")})
    cases = {}
    for name in names:
        pre = name + "/"
        case = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        k = int(case["config"][0])
        case["param"] = {kk[len("param_k%d/" % k):]: z[kk] for kk in z.files if kk.startswith("param_k%d/" % k)}
        cases[name] = case
    return cases


def build(case, device="cpu"):
    from ao_amd.ptv2 import CACSegmentor

    k, c, thr, detach, lovasz, temp = case["config"].tolist()
    seg = CACSegmentor(num_classes=int(k), backbone_out_channels=int(c), backbone=Identity(),
                       criteria=[CE, LOV] if lovasz else [CE], cos_temp=temp, conf_thresh=thr, detach_pre_logits=bool(detach))
    seg.load_state_dict({kk: torch.from_numpy(v.astype(np.float32) if v.dtype == np.float16 else v)
                         for kk, v in case["param"].items()}, strict=True)
    return seg.to(device)


def run_case(case, device="cpu", offset_host=True):
    """one training step and an eval forward: (terms, grads {name: tensor}, feat grad, state after, eval dict)"""
    seg = build(case, device).train()
    feat = torch.from_numpy(case["feat"].astype(np.float32)).to(device).requires_grad_(True)
    data = dict(feat=feat, offset=torch.from_numpy(case["offset"]).to(device), segment=torch.from_numpy(case["segment"]).to(device))
    if offset_host:
        data["offset_host"] = case["offset"].tolist()
    out = seg(data)
    out["loss"].backward()
    terms = {t: float(out[t].detach()) for t in TERMS}
    grads = {n: p.grad.detach().cpu() if p.grad is not None else torch.zeros_like(p).cpu() for n, p in seg.named_parameters()}
    state = {n: v.detach().cpu() for n, v in seg.state_dict().items()}
    seg.eval()
    with torch.no_grad():
        ev = seg(dict(feat=feat.detach(), offset=data["offset"], segment=data["segment"]))
    return terms, grads, feat.grad.detach().cpu(), state, {k: v.detach().cpu() for k, v in ev.items()}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check_against_fixture(case, result, loss_rtol=2e-5, grad_rtol=2e-4):
    terms, grads, gfeat, state, ev = result
    for t in TERMS:
        want = float(case["out/" + t])
        assert abs(terms[t] - want) <= loss_rtol * max(1.0, abs(want)), (t, terms[t], want)
    assert rel_l2(gfeat, case["grad/feat"]) < grad_rtol, rel_l2(gfeat, case["grad/feat"])
    for name, g in grads.items():
        want = case["grad/" + name]
        if not np.any(want):
            assert float(g.abs().max()) < 1e-6, name
            continue
        assert rel_l2(g, want) < grad_rtol, (name, rel_l2(g, want))
    for k in case:
        if k.startswith("after/"):
            name = k[len("after/"):]
            if "num_batches" in name:
                assert int(state[name]) == int(case[k]), (name, int(state[name]), int(case[k]))
            else:
                assert rel_l2(state[name], case[k]) < 1e-5, name
    assert rel_l2(ev["seg_logits"], case["eval/seg_logits"]) < 1e-5
    assert abs(float(ev["loss"]) - float(case["eval/loss"])) <= loss_rtol * abs(float(case["eval/loss"]))


@pytest.fixture(scope="module")
def cases(golden):
    return cac_cases(golden)


def test_fixture_covers_the_cases(cases):
    ks = {int(c["config"][0]) for c in cases.values()}
    thrs = {float(c["config"][2]) for c in cases.values()}
    assert ks == {20, 200} and thrs == {0.0, 0.75}
    assert {bool(c["config"][3]) for c in cases.values()} == {True, False}
    assert {bool(c["config"][4]) for c in cases.values()} == {True, False}
    for c in cases.values():
        assert len(c["offset"]) == 2 and (c["segment"] == -1).any()
        assert len(np.unique(c["segment"][c["segment"] >= 0])) < int(c["config"][0])  # absent classes


@pytest.mark.parametrize("name", ["k20_t075_det_celov", "k200_t0_det_celov", "k20_t0_nodet_ce", "k20_t075_nodet_ce"])
def test_eager_path_matches_the_reference(cases, name):
    case = cases[name]
    check_against_fixture(case, run_case(case))
    # without offset_host: ONE offset.tolist(), same results
    check_against_fixture(case, run_case(case, offset_host=False))


def test_batchnorm_counts_one_update_per_scene_and_one_for_the_batch(cases):
    case = cases["k20_t0_nodet_ce"]
    state = run_case(case)[3]
    assert int(state["feat_proj_layer.1.num_batches_tracked"]) == len(case["offset"]) + 1


def test_state_dict_keys_are_the_reference_keys(cases):
    for case in cases.values():
        seg = build(case)
        assert list(seg.state_dict().keys()) == case["keys"].tolist()


def test_registered_as_cac_v1m1_and_built_from_both_configs():
    from ao_amd.ptv2 import CACSegmentor, registry
    from ao_amd.ptv2.losses import LovaszLoss
    from ao_amd.ptv2.model import PointTransformerV2
    from tests.test_registry_host import Registry

    MODELS = Registry("models")
    registry.register(MODELS=MODELS)
    assert MODELS.get("CAC-v1m1") is CACSegmentor
    for cfg, k, thr in ((SCANNET_CAC, 20, 0.75), (SCANNET200_CAC, 200, 0)):
        seg = MODELS.build(cfg)
        assert isinstance(seg, CACSegmentor) and isinstance(seg.backbone, PointTransformerV2)
        assert seg.backbone.num_classes == 0 and isinstance(seg.backbone.seg_head, torch.nn.Identity)
        assert seg.num_classes == k and seg.conf_thresh == thr and seg.detach_pre_logits is True
        assert tuple(seg.seg_head.weight.shape) == (k, 48)
        assert [lov is not None for _, _, lov in seg._criteria] == [False, True]
        assert isinstance(seg._criteria[1][2], LovaszLoss)


def test_refuses_unsupported_criteria_and_backbones():
    from ao_amd.ptv2 import CACSegmentor

    with pytest.raises(NotImplementedError):
        CACSegmentor(20, 48, backbone=Identity(), criteria=[dict(type="FocalLoss")])
    with pytest.raises(NotImplementedError):
        CACSegmentor(20, 48, backbone=Identity(), criteria=[dict(type="LovaszLoss", loss_weight=1.0)])  # no mode
    with pytest.raises(NotImplementedError):
        CACSegmentor(20, 48, backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0))


def test_distill_loss_is_zero_without_a_labelled_row():
    from ao_amd.ptv2.cac import distill_loss

    pred = torch.randn(50, 20, requires_grad=True)
    loss = distill_loss(pred, torch.randn(50, 20), torch.full((50,), -1, dtype=torch.int64))
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert float(pred.grad.abs().max()) == 0.0
