"""GPU: PointGroup (ao_amd/pointgroup/model.py) -- a training step on spunet_cases.model_batch() on the HIP path against
AO_AMD_PG=torch under the M-rule of tests/test_gpu_spunet_model.py (same backbone, same M per output class), the evaluation
forward against propose(heads(backbone)), propose() against tests/pointgroup_ref.py, and the reference's recorded run
(tests/golden/pointgroup.npz).

The M-rule: |HIP - f64| <= M[output] * max(|AO_AMD_PG=torch - f64|, 2^-24 |f64|) in L2, the float64 run being
tests/spunet_ref.py's backbone with torch heads and the reference's loss statements, in float64 on the same device."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import pointgroup_cases as C
from tests import pointgroup_ref as R
from tests import spunet_cases as SC
from tests import spunet_ref as SR

pytestmark = pytest.mark.gpu

M_MODEL = {"loss": 1, "grad": 8, "buffer": 4}  # tests/test_gpu_spunet_model.py: M_MODEL
FLOOR = 2.0 ** -24
LOSSES = ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _batch():
    """the SpUNet model batch (3 424 points, two clouds) with synthetic segment (5 % ignored), instance (20 % ignored) and
    instance_center"""
    batch = SC.model_batch()
    rng = np.random.default_rng(90)
    n = batch["feat"].shape[0]
    batch["coord"] = np.ascontiguousarray(batch["feat"][:, :3])
    batch["segment"][rng.uniform(size=n) < 0.05] = -1
    batch["instance"] = rng.integers(0, 10, n).astype(np.int64)
    batch["instance"][rng.uniform(size=n) < 0.2] = -1
    batch["instance_center"] = (batch["coord"] + rng.normal(0.0, 0.3, (n, 3))).astype(np.float32)
    assert n == 3424 and batch["offset"].tolist() == [2130, 3424]
    return {k: torch.from_numpy(v).cuda() for k, v in batch.items()}


class _RefPointGroup(nn.Module):
    """the reference's module tree over tests/spunet_ref.py's backbone, for any dtype"""

    def __init__(self):
        super().__init__()
        self.backbone = SR.SpUNet(6, 0)
        self.bias_head = nn.Sequential(nn.Linear(96, 96), nn.BatchNorm1d(96, eps=1e-3, momentum=0.01), nn.ReLU(), nn.Linear(96, 3))
        self.seg_head = nn.Linear(96, 13)

    def forward(self, batch, tables):
        from ao_amd.pointgroup import bias_loss_torch

        feat = self.backbone(batch, tables)
        bias_pred, logit_pred = self.bias_head(feat), self.seg_head(feat)
        seg_loss = torch.nn.functional.cross_entropy(logit_pred, batch["segment"], ignore_index=-1)
        l1, cos = bias_loss_torch(bias_pred, batch["coord"].to(feat.dtype), batch["instance_center"].to(feat.dtype), batch["instance"], -1)
        return dict(loss=seg_loss + l1 + cos, seg_loss=seg_loss, bias_l1_loss=l1, bias_cosine_loss=cos)


def _state():
    return SC.fill_state(SC.shapes_of(_RefPointGroup()), SC.MODEL_SEED)


def _collect(model, out):
    res = {key: out[key].detach() for key in LOSSES}
    res.update({"g:" + k: p.grad for k, p in model.named_parameters()})
    res.update({"b:" + k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")})
    return res


def _ours(path, monkeypatch):
    from ao_amd import pointgroup, spunet

    monkeypatch.setenv("AO_AMD_PG", path)
    model = pointgroup.PointGroup(backbone=spunet.SpUNetBase(6, 0), backbone_out_channels=96, semantic_num_classes=13)
    model.load_state_dict(_state(), strict=True)
    model = model.cuda().train()
    out = model(_batch())
    assert set(out) == set(LOSSES)
    out["loss"].backward()
    return _collect(model, out)


def test_training_step_hip_against_torch(monkeypatch):
    batch = _batch()
    tables = SR.tables_to(SR.build_tables(batch["discrete_coord"].cpu().numpy(), batch["offset"].cpu().numpy()), "cuda")
    ref = _RefPointGroup()
    ref.load_state_dict(_state(), strict=True)
    ref = ref.to(device="cuda", dtype=torch.float64).train()
    out = ref(dict(batch, feat=batch["feat"].double()), tables)
    out["loss"].backward()
    f64 = _collect(ref, out)
    f32, got = _ours("torch", monkeypatch), _ours("hip", monkeypatch)
    assert set(got) == set(f64) == set(f32)
    bad = []
    for key in sorted(got):
        if key.endswith("num_batches_tracked"):
            assert int(got[key]) == int(f64[key]), key
            continue
        assert torch.isfinite(got[key]).all(), key
        kind = "loss" if key in LOSSES else "buffer" if key.startswith("b:") else "grad"
        err = float((got[key].double() - f64[key]).norm())
        allowed = M_MODEL[kind] * max(float((f32[key].double() - f64[key]).norm()), FLOOR * float(f64[key].norm()))
        if kind == "loss" or not err <= allowed:
            print("pointgroup-model-ratio %-6s %-40s f64 %+.6e err %.3e allowed %.3e" % (kind, key, float(f64[key].norm()), err, allowed))
        if not err <= allowed:
            bad.append((key, err, allowed))
    assert all(p.grad is not None for p in ref.parameters()), "the gradient of every parameter"
    assert not bad, bad


def _fixture_model():
    from ao_amd import pointgroup

    with np.load(os.path.join(GOLDEN, "pointgroup.npz")) as f:
        fix = {k: f[k] for k in f.files}

    class Recorded(nn.Module):
        def forward(self, data_dict):
            return data_dict["recorded_feat"]

    model = pointgroup.PointGroup(backbone=Recorded(), backbone_out_channels=16, **C.PROPOSE_CFG)
    model.load_state_dict({k[len("state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("state.")}, strict=True)
    batch = {k: torch.from_numpy(fix[k]).cuda() for k in ("coord", "offset", "segment", "instance", "instance_center")}
    batch["recorded_feat"] = torch.from_numpy(fix["feat"]).cuda()
    return model.cuda(), batch, fix


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_the_references_recorded_run(path, monkeypatch):
    """the reference's forward on the CPU (tests/golden/make_golden_pointgroup.py) against this model on the same inputs and
    weights: masks and classes exactly (the fixture keeps the ball query's margin), scores and losses to fp32 rounding"""
    monkeypatch.setenv("AO_AMD_PG", path)
    model, batch, fix = _fixture_model()
    for mode in ("train", "eval"):
        model.train(mode == "train")
        with torch.no_grad():
            out = model(dict(batch))
        for key in LOSSES:
            want = float(fix["%s.%s" % (mode, key)])
            assert abs(float(out[key]) - want) <= 4e-6 * max(abs(want), 1.0), (mode, key, float(out[key]), want)
        if mode == "train":
            assert set(out) == set(LOSSES)
            model.load_state_dict({k[len("state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("state.")}, strict=True)
    for key in ("pred_scores", "pred_masks", "pred_classes"):
        assert not out[key].is_cuda and out[key].dtype == torch.from_numpy(fix[key]).dtype and out[key].shape == fix[key].shape, key
    assert np.array_equal(out["pred_masks"].numpy(), fix["pred_masks"]) and np.array_equal(out["pred_classes"].numpy(), fix["pred_classes"])
    assert np.abs(out["pred_scores"].numpy() - fix["pred_scores"]).max() <= 1e-6
    # forward in evaluation is exactly propose(heads(backbone(...)))
    with torch.no_grad():
        scores, masks, classes = model.propose(batch["coord"], batch["offset"], *model.heads(model.backbone(batch)))
    assert torch.equal(scores, out["pred_scores"]) and torch.equal(masks, out["pred_masks"]) and torch.equal(classes, out["pred_classes"])
    assert scores.shape == (8,)


def test_evaluation_forward_on_the_model_batch(monkeypatch):
    """the whole model in evaluation mode: the losses and the three outputs, which equal propose(heads(backbone)) bit for bit"""
    from ao_amd import pointgroup, spunet

    monkeypatch.setenv("AO_AMD_PG", "hip")
    model = pointgroup.PointGroup(backbone=spunet.SpUNetBase(6, 0), backbone_out_channels=96, semantic_num_classes=13,
                                  segment_ignore_index=(-1, 0), cluster_min_points=5, cluster_propose_points=10, voxel_size=0.05)
    model.load_state_dict(_state(), strict=True)
    model, batch = model.cuda().eval(), _batch()
    with torch.no_grad():
        out = model(batch)
        scores, masks, classes = model.propose(batch["coord"], batch["offset"], *model.heads(model.backbone(batch)))
    assert set(out) == set(LOSSES) | {"pred_scores", "pred_masks", "pred_classes"}
    assert torch.equal(scores, out["pred_scores"]) and torch.equal(masks, out["pred_masks"]) and torch.equal(classes, out["pred_classes"])
    assert masks.shape[1] == 3424 and masks.dtype == torch.int32 and classes.dtype == torch.int64 and scores.dtype == torch.float32
    assert not masks.is_cuda and all(torch.isfinite(out[k]) for k in LOSSES)
    print("pointgroup-model eval proposals on the model batch:", masks.shape[0], masks.sum(1).tolist())


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_propose_against_the_restatement(path, monkeypatch):
    """blobs of 60, 101 and 150 points around three centres, in two clouds, with one ignored class"""
    from ao_amd import pointgroup

    monkeypatch.setenv("AO_AMD_PG", path)
    coord, offset, bias, logit = C.propose_case()
    cfg = C.PROPOSE_CFG
    want_scores, want_masks, want_classes, members, margin = R.propose(
        coord, offset, bias, logit, cfg["segment_ignore_index"], cfg["cluster_thresh"], cfg["cluster_min_points"],
        cfg["cluster_propose_points"], cfg["voxel_size"])
    assert margin > C.MARGIN, "the ball query's margin"
    assert sorted(members.tolist()) == [101, 101, 150, 150] and sorted(want_classes.tolist()) == [2, 2, 3, 3]
    model = pointgroup.PointGroup(backbone=nn.Identity(), backbone_out_channels=8, **cfg).cuda().eval()
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    scores, masks, classes = model.propose(dev(coord), dev(offset), dev(bias), dev(logit))
    assert np.array_equal(masks.numpy(), want_masks) and np.array_equal(classes.numpy(), want_classes)
    rel = np.abs(scores.numpy().astype(np.float64) - want_scores) / want_scores
    print("pointgroup-propose", path, "relative score error", rel, "bound", (members + 8) * 2.0 ** -24)
    assert (rel <= (members + 8) * 2.0 ** -24).all()
    # no point survives segment_ignore_index: the reference raises, this returns empty outputs
    none = pointgroup.PointGroup(backbone=nn.Identity(), backbone_out_channels=8, **dict(cfg, segment_ignore_index=(0, 1, 2, 3, 4)))
    scores, masks, classes = none.cuda().eval().propose(dev(coord), dev(offset), dev(bias), dev(logit))
    assert scores.shape == (0,) and masks.shape == (0, 702) and classes.shape == (0,)
    assert masks.dtype == torch.int32 and classes.dtype == torch.int64 and scores.dtype == torch.float32
