"""CPU: LovaszLoss(mode="multiclass") criteria in DefaultSegmentor, the eager formulation of ao_amd/ptv2/losses.py against the
reference's own output (tests/golden/lovasz.npz, generator tests/golden/make_golden_lovasz.py running
pointcept/models/losses/lovasz.py), and the LOSSES registration.  The HIP path runs in tests/test_gpu_lovasz.py."""
import numpy as np
import pytest
import torch

from tests.test_registry_host import Registry


def lovasz_cases(golden):
    g = golden("lovasz.npz")
    out = {}
    for name in [str(s) for s in g["cases"]]:
        d = {k.split("__", 1)[1]: g[k] for k in g.files if k.startswith(name + "__")}
        src = str(d["inputs_of"]) if "inputs_of" in d else name
        logits = torch.from_numpy(g[src + "__logits"])
        label = torch.from_numpy(g[src + "__label"].astype(np.int64))
        seen = [int(v) for v in d["class_seen"]] if int(d["has_class_seen"]) else None
        out[name] = dict(logits=logits, label=label, ignore_index=int(d["ignore_index"]), class_seen=seen,
                         loss_weight=float(d["loss_weight"]), loss=float(d["loss"]), grad=torch.from_numpy(d["grad"]))
    return out


def check_against_fixture(case, loss, grad):
    assert abs(float(loss) - case["loss"]) <= 1e-6 * abs(case["loss"]), (float(loss), case["loss"])
    ref = case["grad"].double()
    rel = float((grad.double().cpu() - ref).norm() / ref.norm())
    assert rel <= 1e-5, rel


def test_eager_path_matches_the_reference(golden):
    from ao_amd.ptv2 import LovaszLoss

    cases = lovasz_cases(golden)
    assert sorted(cases) == ["c13absent", "c20", "c20seen", "one_row", "w05_i255"]
    for name, case in cases.items():
        crit = LovaszLoss(mode="multiclass", class_seen=case["class_seen"], ignore_index=case["ignore_index"],
                          loss_weight=case["loss_weight"])
        x = case["logits"].clone().requires_grad_(True)
        loss = crit(x, case["label"])
        assert loss.dim() == 0
        loss.backward()
        check_against_fixture(case, loss.detach(), x.grad)


def test_eager_edge_cases():
    from ao_amd.ptv2 import lovasz_softmax

    x = torch.randn(50, 6, requires_grad=True)
    none = torch.full((50,), -1, dtype=torch.int64)
    loss = lovasz_softmax(x, none, -1)  # no labelled row: a 0-dim zero, zero gradient
    assert loss.dim() == 0 and float(loss.detach()) == 0.0
    loss.backward()
    assert torch.count_nonzero(x.grad) == 0
    lab = torch.randint(0, 3, (50,))
    assert float(lovasz_softmax(x, lab, -1, class_seen=[4, 5])) == 0.0  # no class left after class_seen
    bad = lab.clone()
    bad[7] = 9
    assert torch.isnan(lovasz_softmax(x, bad, -1))
    assert torch.isfinite(lovasz_softmax(x, bad, 9))  # fine when that IS the ignore_index
    assert torch.isfinite(lovasz_softmax(x, lab, None))  # ignore_index=None: every row
    with pytest.raises(ValueError):
        lovasz_softmax(torch.randn(5, 1), torch.zeros(5, dtype=torch.int64), -1)  # C == 1, as lovasz.py:135-137


def test_check_labels_switch_raises(monkeypatch):
    from ao_amd.ptv2 import lovasz_softmax

    monkeypatch.setenv("AO_AMD_CHECK_LABELS", "1")
    lab = torch.randint(0, 3, (20,))
    lab[3] = 12
    with pytest.raises(ValueError):
        lovasz_softmax(torch.randn(20, 4), lab, -1)


class _FixedBackbone(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(logits.clone())

    def forward(self, input_dict):
        return self.logits


def test_segmentor_sums_ce_and_lovasz_in_config_order(golden):
    """The criteria line of configs/scannet/semseg-pt-v2m2-3-lovasz.py:37-40 builds and sums as the reference's Criteria."""
    from ao_amd.ptv2 import DefaultSegmentor, LovaszLoss

    case = lovasz_cases(golden)["c20"]
    criteria = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    seg = DefaultSegmentor(_FixedBackbone(case["logits"]), criteria=criteria).train()
    assert seg.ignore_index == -1
    batch = dict(segment=case["label"])
    loss = seg(batch)["loss"]
    ce = torch.nn.functional.cross_entropy(case["logits"], case["label"], ignore_index=-1)
    assert abs(float(loss) - (float(ce) + case["loss"])) < 2e-6
    loss.backward()
    x = case["logits"].clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(x, case["label"], ignore_index=-1).backward()
    check_against_fixture(dict(case, loss=case["loss"], grad=case["grad"] + x.grad), torch.tensor(case["loss"]),
                          seg.backbone.logits.grad)
    # loss_weight and class_seen reach the Lovasz term; the state dict is the CE-only one
    half = DefaultSegmentor(_FixedBackbone(case["logits"]), criteria=[
        dict(type="LovaszLoss", mode="multiclass", loss_weight=0.5, ignore_index=-1, class_seen=[0, 2, 3])]).eval()
    want = 0.5 * float(LovaszLoss("multiclass", class_seen=[0, 2, 3], ignore_index=-1)(case["logits"], case["label"]))
    assert abs(float(half(batch)["loss"]) - want) < 1e-7
    assert sorted(half.state_dict()) == sorted(DefaultSegmentor(_FixedBackbone(case["logits"])).state_dict())


@pytest.mark.parametrize("cfg, exc", [
    (dict(type="LovaszLoss"), NotImplementedError),  # the reference's constructor requires mode
    (dict(type="LovaszLoss", mode="binary"), NotImplementedError),
    (dict(type="LovaszLoss", mode="multilabel", ignore_index=-1), NotImplementedError),
    (dict(type="LovaszLoss", mode="multiclass", per_image=True), NotImplementedError),
    (dict(type="LovaszLoss", mode="multiclass", smooth=0.1), NotImplementedError),
    (dict(type="LovaszLoss", mode="softmax"), ValueError),
    (dict(type="DiceLoss"), NotImplementedError),
])
def test_refused_criteria(cfg, exc):
    from ao_amd.ptv2 import DefaultSegmentor

    with pytest.raises(exc):
        DefaultSegmentor(_FixedBackbone(torch.zeros(4, 3)), criteria=[dict(type="CrossEntropyLoss"), cfg])


@pytest.mark.parametrize("cfg", [
    dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1),  # scannet / scannet200 / semantic_kitti
    dict(type="LovaszLoss", mode="multiclass", class_seen=[1, 2], per_image=False, ignore_index=None, loss_weight=2.0),
])
def test_accepted_lovasz_criteria(cfg):
    from ao_amd.ptv2 import DefaultSegmentor, LovaszLoss

    seg = DefaultSegmentor(_FixedBackbone(torch.zeros(4, 3)), criteria=[dict(type="CrossEntropyLoss"), cfg])
    (_, _, first), (w, ig, lov) = seg._criteria
    assert first is None and isinstance(lov, LovaszLoss)
    assert w == cfg["loss_weight"] and ig == cfg["ignore_index"] and lov.class_seen == cfg.get("class_seen")
    assert seg.ignore_index == -1


def test_sam_segmentor_inherits_lovasz_criteria(golden):
    from ao_amd.ptv2 import DefaultSegmentorSAM_Image

    case = lovasz_cases(golden)["c13absent"]
    seg = DefaultSegmentorSAM_Image(_FixedBackbone(case["logits"]), criteria=[
        dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]).eval()
    assert abs(float(seg(dict(segment=case["label"]))["loss"]) - case["loss"]) <= 1e-6 * case["loss"]


def test_lovasz_registers_under_the_reference_losses_registry(golden):
    """registry.register(LOSSES=...): the reference's Criteria (losses/builder.py:13-29) builds the entry from the config
    line and sums it; the other registries' meaning is unchanged."""
    from ao_amd.ptv2 import registry
    from ao_amd.ptv2.losses import LovaszLoss

    LOSSES = Registry("losses")
    assert registry.register(LOSSES=LOSSES) == ["LovaszLoss"]
    assert LOSSES.get("LovaszLoss") is LovaszLoss
    MODELS, OPTIMIZERS = Registry("models"), Registry("optimizers")
    assert set(registry.register(MODELS=MODELS, OPTIMIZERS=OPTIMIZERS)) == {"PT-v2m2", "DefaultSegmentor",
                                                                             "DefaultSegmentorSAM_Image", "FlatAdamW"}
    assert LOSSES.get("CrossEntropyLoss") is None
    case = lovasz_cases(golden)["w05_i255"]
    crit = LOSSES.build(dict(type="LovaszLoss", mode="multiclass", loss_weight=0.5, ignore_index=255))
    loss = 0
    for c in [crit]:  # Criteria.__call__
        loss += c(case["logits"], case["label"])
    assert abs(float(loss) - case["loss"]) <= 1e-6 * case["loss"]
    registry.register(LOSSES=LOSSES)  # re-registration replaces
    with pytest.raises(KeyError):
        registry.register(LOSSES=LOSSES, force=False)
