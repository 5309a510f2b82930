"""GPU: the instance evaluator's association (ao_amd/pointgroup/evaluate.py on ao_amd/csrc/inseval.hip)
against the reference's recorded run and the brute-force restatement of tests/inseval_ref.py.  Every output is an integer count
or a widened fp32 score: every array of every record is compared for equality, nothing is left out."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import inseval_cases as C
from tests import inseval_ref as R
from tests import pointgroup_cases as PC
from tests.test_inseval_host import assert_record, recorded

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "inseval.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def scenes():
    return C.scenes()


def _consts():
    from ao_amd import _abi

    return _abi.inseval_consts["INSEVAL_POINTS_PER_WG"], _abi.inseval_consts["INSEVAL_BINS"]


def _associate(masks, scores, classes, segment, instance, nn_idx=None, masks_on="cuda", ignore=C.SEGMENT_IGNORE, min_region=C.MIN_REGION):
    from ao_amd.pointgroup import associate

    masks = torch.from_numpy(masks)
    pred = dict(pred_masks=masks.cuda() if masks_on == "cuda" else masks, pred_scores=torch.from_numpy(scores),
                pred_classes=torch.from_numpy(classes))
    return associate(pred, torch.from_numpy(segment).cuda(), torch.from_numpy(instance).cuda(), C.NUM_CLASSES, ignore,
                     C.INSTANCE_IGNORE, min_region, None if nn_idx is None else torch.from_numpy(nn_idx).cuda())


@pytest.mark.parametrize("masks_on", ["cuda", "cpu"])
@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", C.SCENES)
def test_the_references_recorded_scenes(fixture, scenes, name, path, masks_on, monkeypatch):
    monkeypatch.setenv("AO_AMD_INSEVAL", path)
    s = scenes[name]
    got = _associate(s["masks"], s["scores"], s["classes"], s["segment"], s["instance"], masks_on=masks_on)
    assert_record(got, recorded(fixture, name), (name, path, masks_on))


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_origin_mapping(path, monkeypatch):
    """6 000 origin points read the 4 000-point masks through nn_idx: the reference's pred_masks[:, idx], never formed here"""
    monkeypatch.setenv("AO_AMD_INSEVAL", path)
    s, nn_idx, segment, instance = C.origin_case()
    assert nn_idx.shape == (6000,) and s["masks"].shape[1] == 4000
    want = R.associate(s["masks"][:, nn_idx], s["scores"], s["classes"], segment, instance, C.SEGMENT_IGNORE, C.INSTANCE_IGNORE, C.MIN_REGION)
    assert want["inter"].shape[0] >= 8 and want["inter"].shape[1] >= 5 and want["pred_void"].max() > 0
    got = _associate(s["masks"], s["scores"], s["classes"], segment, instance, nn_idx)
    assert_record(got, want, path)


def _random_case(seed, p, n, g):
    """p proposals of density 0.3 with values 1, 2, -1 over n points of g instances (non-contiguous ids; every id present when
    n >= g, its first point neither void nor without a class), a tenth of the other points void, a tenth without instance"""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, max(g, 1), n)
    col[:min(g, n)] = np.arange(min(g, n))
    instance = (col * 3 + 1).astype(np.int64)
    segment = (col % 3 + 1).astype(np.int64)
    free = np.arange(n) >= g
    segment[free & (rng.uniform(size=n) < 0.1)] = -1
    instance[free & (rng.uniform(size=n) < 0.1)] = -1
    if g == 0:
        instance[:] = -1
    masks = ((rng.uniform(size=(p, n)) < 0.3) * rng.choice([1, 2, -1], (p, n))).astype(np.int32)
    classes = rng.integers(0, 4, p).astype(np.int64)
    classes[:1] = 1  # (class 0 is ignored: the first proposal is always kept)
    return masks, rng.uniform(size=p).astype(np.float32), classes, segment, instance


def _shape_cases():
    pts, bins = _consts()
    return {"n=wg": (5, pts, 7), "n=wg-1": (5, pts - 1, 7), "n=wg+1": (5, pts + 1, 7), "n=1": (3, 1, 1), "P=1": (1, 700, 9),
            "P=0": (0, 300, 4), "G=0": (6, 500, 0), "windows": (6, 3 * (bins + 3), bins + 3)}


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("case", ["n=wg", "n=wg-1", "n=wg+1", "n=1", "P=1", "P=0", "G=0", "windows"])
def test_shapes(case, path, monkeypatch):
    """one workgroup exactly, one point less and one more; one point; one proposal; none; no ground truth; more ground truths
    than one call's bins.  min_region_size 0 keeps every proposal of a class that is not ignored."""
    monkeypatch.setenv("AO_AMD_INSEVAL", path)
    p, n, g = _shape_cases()[case]
    masks, scores, classes, segment, instance = _random_case(11, p, n, g)
    want = R.associate(masks, scores, classes, segment, instance, C.SEGMENT_IGNORE, C.INSTANCE_IGNORE, 0)
    assert want["inter"].shape == (int((classes != 0).sum()), g if n >= g else n)
    if case == "windows":
        assert g == _consts()[1] + 3 and n == 3 * g and want["inter"][:, -3:].sum() > 0, "the last window holds counts"
    got = _associate(masks, scores, classes, segment, instance, min_region=0)
    assert_record(got, want, (case, path))
    if case == "P=0":
        assert got.inter.shape == (0, 4) and got.pred_row.shape == (0,) and got.gt_vert_count.sum() > 0
    if case == "G=0":
        assert got.inter.shape[1] == 0 and got.inter.shape[0] > 0 and got.pred_vert_count.min() > 0


def test_worst_contention():
    """every lane of every wave adds into one bin: masks all set, one ground truth, four workgroups of points"""
    pts, _ = _consts()
    n = 4 * pts
    masks = np.full((3, n), 5, np.int32)
    got = _associate(masks, np.array([0.5, 0.25, 0.125], np.float32), np.array([1, 1, 2], np.int64), np.ones(n, np.int64),
                     np.full(n, 9, np.int64))
    assert got.inter.tolist() == [[n], [n], [n]] and got.pred_vert_count.tolist() == [n] * 3 and got.pred_void.tolist() == [0] * 3
    assert got.gt_vert_count.tolist() == [n] and got.pred_conf.tolist() == [0.5, 0.25, 0.125]


def _fixture_model(cloud):
    """a tiny PointGroup over the recorded features of one cloud of tests/golden/pointgroup.npz (its backbone returns them)"""
    from ao_amd import pointgroup

    with np.load(os.path.join(GOLDEN, "pointgroup.npz")) as f:
        fix = {k: f[k] for k in f.files}

    class Recorded(nn.Module):
        def forward(self, data_dict):
            return data_dict["recorded_feat"]

    model = pointgroup.PointGroup(backbone=Recorded(), backbone_out_channels=16, **PC.PROPOSE_CFG)
    model.load_state_dict({k[len("state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("state.")}, strict=True)
    ends = [0] + fix["offset"].tolist()
    sel = slice(ends[cloud], ends[cloud + 1]) if cloud is not None else slice(0, ends[-1])
    batch = {k: torch.from_numpy(fix[k][sel]).cuda() for k in ("coord", "segment", "instance", "instance_center")}
    batch["recorded_feat"] = torch.from_numpy(fix["feat"][sel]).cuda()
    batch["offset"] = torch.tensor([ends[cloud + 1] - ends[cloud]] if cloud is not None else ends[1:]).cuda()
    return model.cuda().eval(), batch


def test_propose_device_is_propose_before_the_download():
    model, batch = _fixture_model(None)
    with torch.no_grad():
        heads = model.heads(model.backbone(batch))
    dev = model.propose_device(batch["coord"], batch["offset"], *heads)
    cpu = model.propose(batch["coord"], batch["offset"], *heads)
    assert dev[1].shape == (8, 1462)
    for d, c in zip(dev, cpu):
        assert d.is_cuda and not c.is_cuda and d.dtype == c.dtype and torch.equal(d.cpu(), c)


@pytest.mark.parametrize("origin", [False, True])
def test_evaluate_scene(origin):
    """one cloud through InsSegEvaluator.evaluate_scene: the record that the restatement gives for the model's own proposals"""
    from ao_amd.pointgroup import InsSegEvaluator

    model, batch = _fixture_model(0)
    n = batch["coord"].shape[0]
    with torch.no_grad():
        out = model(dict(batch))
    scores, masks, classes = (out[k].numpy() for k in ("pred_scores", "pred_masks", "pred_classes"))
    assert masks.shape[0] >= 3 and masks.shape[1] == n
    segment, instance = batch["segment"].cpu().numpy(), batch["instance"].cpu().numpy()
    if origin:  # 1 000 origin points that are points of the cloud: each is its own nearest neighbour
        assert len(np.unique(batch["coord"].cpu().numpy(), axis=0)) == n
        sel = np.random.default_rng(3).integers(0, n, 1000)
        batch.update(origin_coord=batch["coord"][sel], origin_offset=torch.tensor([1000]).cuda(),
                     origin_segment=batch["segment"][sel], origin_instance=batch["instance"][sel])
        masks, segment, instance = masks[:, sel], segment[sel], instance[sel]
    ev = InsSegEvaluator(segment_ignore_index=(-1,), instance_ignore_index=-1)
    min_region = 30 if origin else 100
    ev.min_region_sizes = min_region
    want = R.associate(masks, scores, classes, segment, instance, (-1,), -1, min_region)
    assert want["inter"].shape[0] >= 3 and want["inter"].shape[1] >= 3 and (want["inter"] > 0).sum() >= 3
    loss, got = ev.evaluate_scene(model, batch, num_classes=5)
    assert_record(got, want, origin)
    assert abs(loss - float(out["loss"])) <= 1e-6 * max(1.0, abs(float(out["loss"])))
