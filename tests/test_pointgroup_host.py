"""CPU: the host side of PointGroup (ao_amd/pointgroup, include/ptv2_pg_hip.h): the numpy restatement
against the reference's recorded run, the state dict, the header's binding, the host search, the refusals, the registry and
InstanceParser."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import pointgroup_cases as C
from tests import pointgroup_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    with np.load(os.path.join(GOLDEN, "pointgroup.npz")) as f:
        return {k: f[k] for k in f.files}


def _heads64(fix, training):
    """bias_pred, logit_pred of the recorded feat in float64: Linear, BatchNorm1d(eps=1e-3), ReLU, Linear; Linear"""
    w = {k[len("state."):]: v.astype(np.float64) for k, v in fix.items() if k.startswith("state.")}
    x = fix["feat"].astype(np.float64) @ w["bias_head.0.weight"].T + w["bias_head.0.bias"]
    mean, var = (x.mean(0), x.var(0)) if training else (w["bias_head.1.running_mean"], w["bias_head.1.running_var"])
    x = np.maximum((x - mean) / np.sqrt(var + 1e-3) * w["bias_head.1.weight"] + w["bias_head.1.bias"], 0.0)
    return (x @ w["bias_head.3.weight"].T + w["bias_head.3.bias"],
            fix["feat"].astype(np.float64) @ w["seg_head.weight"].T + w["seg_head.bias"])


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_ref_reproduces_the_fixture(mode):
    """tests/pointgroup_ref.py on the fixture's inputs gives what the reference's forward recorded"""
    fix = _fixture()
    assert fix["coord"].shape == (1462, 3) and fix["offset"].tolist() == [731, 1462]
    bias_pred, logit_pred = _heads64(fix, mode == "train")
    l1, cos, _ = R.bias_loss(bias_pred, fix["coord"], fix["instance_center"], fix["instance"], -1)
    logp = np.log(R.softmax64(logit_pred))
    seg = -logp[np.arange(logp.shape[0]), fix["segment"]].mean()  # (no label of the fixture is ignored)
    assert (fix["segment"] >= 0).all()
    for key, value in (("seg_loss", seg), ("bias_l1_loss", l1), ("bias_cosine_loss", cos), ("loss", seg + l1 + cos)):
        want = float(fix["%s.%s" % (mode, key)])
        assert abs(value - want) <= 2e-6 * max(abs(want), 1.0), (key, value, want)
    if mode == "eval":
        cfg = C.PROPOSE_CFG
        scores, masks, classes, members, margin = R.propose(
            fix["coord"], fix["offset"], bias_pred.astype(np.float32), logit_pred.astype(np.float32), cfg["segment_ignore_index"],
            cfg["cluster_thresh"], cfg["cluster_min_points"], cfg["cluster_propose_points"], cfg["voxel_size"])
        assert margin > C.MARGIN
        assert fix["pred_masks"].shape == (8, 1462) and fix["pred_masks"].dtype == np.int32
        assert np.array_equal(masks, fix["pred_masks"]) and np.array_equal(classes, fix["pred_classes"])
        assert sorted(members.tolist()) == [101, 101, 120, 120, 150, 150, 200, 200]
        assert np.abs(scores - fix["pred_scores"]).max() <= 1e-6


def test_manifest_and_strict_loading():
    from ao_amd import pointgroup, spunet

    with open(os.path.join(GOLDEN, "pointgroup_manifest.json")) as f:
        manifest = json.load(f)
    model = pointgroup.PointGroup(backbone_out_channels=96)
    have = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert have == manifest and list(have) == list(manifest), "the reference's keys in the reference's order"
    assert len(manifest) == 354 + 11 and isinstance(model.backbone, spunet.SpUNetBase) and model.backbone.num_classes == 0
    heads = [k for k in manifest if not k.startswith("backbone.")]
    assert heads == ["bias_head.0.weight", "bias_head.0.bias", "bias_head.1.weight", "bias_head.1.bias", "bias_head.1.running_mean",
                     "bias_head.1.running_var", "bias_head.1.num_batches_tracked", "bias_head.3.weight", "bias_head.3.bias",
                     "seg_head.weight", "seg_head.bias"]
    assert manifest["bias_head.3.weight"] == [3, 96] and manifest["seg_head.weight"] == [20, 96]
    assert model.bias_head[1].eps == 1e-3 and model.bias_head[1].momentum == 0.01
    # strict loading of the fixture's head weights over a module backbone
    fix = _fixture()
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("state.")}
    small = pointgroup.PointGroup(backbone=torch.nn.Identity(), backbone_out_channels=16, **C.PROPOSE_CFG)
    small.load_state_dict(state, strict=True)
    for key, value in small.state_dict().items():
        assert torch.equal(value, state[key]), key
    # a config dict resolves to SpUNet-v1m1 with num_classes = 0, whatever it says
    cfg = dict(type="SpUNet-v1m1", in_channels=4, num_classes=13, base_channels=32, channels=(32, 64, 64, 32), layers=(1, 1, 1, 1))
    model = pointgroup.PointGroup(backbone=cfg, backbone_out_channels=32)
    assert model.backbone.num_classes == 0 and model.backbone.in_channels == 4
    with pytest.raises(ValueError, match="backbone type"):
        pointgroup.PointGroup(backbone=dict(type="PT-v2m2"))


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    names = {"ptv2_pg_abi_version", "ptv2_pg_struct_bytes", "ptv2_pg_ballquery_workspace_bytes", "pg_ballquery_count_hip_launcher",
             "pg_ballquery_fill_hip_launcher", "ptv2_pg_cluster_workspace_bytes", "pg_cluster_hip_launcher", "pg_bfs_cluster_host",
             "ptv2_pg_proposals_workspace_bytes", "pg_proposals_count_hip_launcher", "pg_proposals_fill_hip_launcher",
             "ptv2_pg_bias_loss_workspace_bytes", "pg_bias_loss_fwd_hip_launcher", "pg_bias_loss_bwd_hip_launcher"}
    assert set(_abi.pg_signatures) == names
    with open(_abi.PG_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.pg_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_pg_abi_version() == _lib.EXPECTED_PG_ABI == 1
    assert L.ptv2_pg_struct_bytes(0) == ctypes.sizeof(_abi.pg_structs["pg_csr"]) == 24 and L.ptv2_pg_struct_bytes(1) == -1
    assert _abi.pg_consts["PG_BALL_CAP"] == 1000 == R.BALL_CAP
    # the other headers are as they were
    assert _lib.EXPECTED_ABI == 11 and L.ptv2_abi_version() == 11 and L.ptv2_ptv1_abi_version() == 1
    assert L.ptv2_spconv_abi_version() == 1 and L.ptv2_pp2s_abi_version() == 1 and L.ptv2_refine_abi_version() == 1
    assert L.ptv2_data_abi_version() == 1
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert "ptv2_pg_hip.h" in f.read(), "the build digest covers the header"


def test_workspace_queries():
    from ao_amd import _lib

    L = _lib.lib()
    # the cell table is bounded by the number of points (4 cells per point), never by the bounding box: the query takes no
    # coordinates at all, and the `outlier` case (500 points in a unit box, one at 1e6) stays within the bound for 501 points:
    # per point 4 cells * 2 tables * 4 B, four sort arrays, one float4, two counts; per call the scan / sort scratch
    coords, offsets, _ = C.ball_cases()["outlier"]
    assert coords.shape[0] == 501 and float(coords.max()) == 1e6
    per_point = 4 * 2 * 4 + 4 * 4 + 16 + 2 * 4
    assert 0 < L.ptv2_pg_ballquery_workspace_bytes(501, 1) <= 501 * per_point + (1 << 16)
    big = L.ptv2_pg_ballquery_workspace_bytes(150000, 2)
    assert 0 < big <= 150000 * per_point + (1 << 22)
    for bad in ((0, 1), (-5, 1), (100, 0), (100, 1025), (1 << 40, 1)):
        assert L.ptv2_pg_ballquery_workspace_bytes(*bad) == -1, bad
    assert L.ptv2_pg_cluster_workspace_bytes(0) == -1 and 0 < L.ptv2_pg_cluster_workspace_bytes(150000) <= 150000 * 24 + (1 << 22)
    assert L.ptv2_pg_proposals_workspace_bytes(0, 0) == -1 and L.ptv2_pg_proposals_workspace_bytes(10, 11) == -1
    assert L.ptv2_pg_proposals_workspace_bytes(10, -1) == -1 and L.ptv2_pg_proposals_workspace_bytes(150000, 60) > 0
    assert L.ptv2_pg_bias_loss_workspace_bytes(0) == -1 and 0 < L.ptv2_pg_bias_loss_workspace_bytes(10 ** 8) <= 1 << 16


@pytest.mark.parametrize("name", ["chain", "labels_touching", "threshold", "interleaved", "capped_directed", "all_ignored"])
def test_bfs_cluster_equals_the_restatement(name):
    """the drop-in `bfs_cluster` on CPU tensors: the rows in the order of the reference's search"""
    from ao_amd import pointgroup

    _, _, _, label, min_points = C.cluster_cases()[name]
    idx, start_len, capped, rows, offsets, _ = C.cluster_expected(name)
    assert capped == (name == "capped_directed")
    got_rows, got_offsets = pointgroup.bfs_cluster(torch.from_numpy(label), torch.from_numpy(idx), torch.from_numpy(start_len), min_points)
    assert got_rows.dtype == torch.int32 and got_offsets.dtype == torch.int32 and got_rows.shape == (rows.shape[0], 2)
    assert np.array_equal(got_rows.numpy(), rows) and np.array_equal(got_offsets.numpy(), offsets)
    if name == "capped_directed":
        # one cluster of the 1 000 lowest blob indices; the other 100 blob points seed searches that reach only visited points
        is_blob = C.cap_case(1100)[3]
        assert offsets.tolist() == [0, 1000] and np.array_equal(np.sort(rows[:, 1]), np.nonzero(is_blob)[0][:1000])
    if name == "chain":
        assert rows[0, 1] == 0 and offsets.tolist() == [0, 200]
    if name == "threshold":
        assert sorted(np.diff(offsets).tolist()) == [10, 11], "min_points - 1 is dropped, min_points kept"
    if name == "all_ignored":
        assert got_rows.shape == (0, 2) and got_offsets.tolist() == [0]


def test_bfs_cluster_refuses_bad_lists():
    from ao_amd import pointgroup

    label = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="outside"):
        pointgroup.bfs_cluster(label, torch.tensor([0, 1, 7], dtype=torch.int32), torch.tensor([[0, 1], [1, 1], [2, 1]], dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="outside"):
        pointgroup.bfs_cluster(label, torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([[0, 1], [1, 1], [2, 2]], dtype=torch.int32), 1)


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_no_cpu_fallback(path, monkeypatch):
    from ao_amd import pointgroup

    monkeypatch.setenv("AO_AMD_PG", path)
    coords, offsets, radius = C.ball_cases()["lattice_strict"]
    coords, offsets = torch.from_numpy(coords), torch.from_numpy(offsets)
    batch = torch.zeros(coords.shape[0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointgroup.ballquery_batch_p(coords, batch, offsets, radius, 300)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointgroup.ball_query(coords, offsets, radius)
    idx, start_len, _, _, _, pc = C.cluster_expected("threshold")
    label = torch.ones(30, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointgroup.cluster(label, torch.from_numpy(idx), torch.from_numpy(start_len), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointgroup.proposals(torch.from_numpy(pc), torch.tensor([11, 10], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
                             torch.zeros(30, dtype=torch.int64), torch.rand(30, 4), 5)
    pred, coord, center, instance = (torch.from_numpy(v) for v in C.loss_case(300, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointgroup.bias_loss(pred, coord, center, instance, -1)
    model = pointgroup.PointGroup(backbone=torch.nn.Identity(), backbone_out_channels=16, **C.PROPOSE_CFG).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.propose(coord, torch.tensor([300]), pred, torch.rand(300, 5))


def test_dropin_name():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "dropin"))
    try:
        import pointgroup_ops
        from ao_amd.pointgroup import ops

        assert pointgroup_ops.ballquery_batch_p is ops.ballquery_batch_p and pointgroup_ops.bfs_cluster is ops.bfs_cluster
    finally:
        sys.path.remove(os.path.join(root, "dropin"))
        sys.modules.pop("pointgroup_ops", None)


def test_registry_files_the_name():
    from ao_amd import pointgroup
    from ao_amd.ptv2 import registry

    class Fake:
        def __init__(self):
            self.modules = {}

        def register_module(self, module=None, name=None, force=False):
            self.modules[name] = module

    fake = Fake()
    done = registry.register(MODELS=fake)
    assert done == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image"], "filed and not listed"
    assert fake.modules["PG-v1m1"] is pointgroup.PointGroup


def _instance_parser_numpy(coord, segment, instance, segment_ignore, ignore):
    """the reference's loop over the instances"""
    instance = instance.copy()
    mask = ~np.isin(segment, segment_ignore)
    instance[~mask] = ignore
    unique, inverse = np.unique(instance[mask], return_inverse=True)
    instance[mask] = inverse
    center = np.ones((coord.shape[0], 3)) * ignore
    bbox = np.ones((len(unique), 6)) * ignore
    for i in range(len(unique)):
        sel = instance == i
        center[sel] = coord[sel].astype(np.float64).mean(0)
        bbox[i] = np.concatenate([coord[sel].min(0), coord[sel].max(0)])
    return instance, center, bbox


def test_instance_parser():
    """3 instances and one ignored class, on CPU tensors"""
    from ao_amd.ptv2.transform import InstanceParser

    rng = np.random.default_rng(0)
    n = 200
    coord = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    instance = rng.choice([4, 9, 17], n).astype(np.int64)
    segment = np.where(instance == 4, 2, np.where(instance == 9, 5, 3)).astype(np.int64)
    ignored = rng.uniform(size=n) < 0.25
    segment[ignored] = 1  # the ignored class: its points keep an instance id that must not survive
    want_instance, want_center, want_bbox = _instance_parser_numpy(coord, segment, instance, (-1, 0, 1), -1)
    assert want_bbox.shape == (3, 6) and (want_instance[ignored] == -1).all()
    out = InstanceParser(segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1)(
        dict(coord=torch.from_numpy(coord), segment=torch.from_numpy(segment), instance=torch.from_numpy(instance.copy())))
    assert out["instance"].dtype == torch.int64 and np.array_equal(out["instance"].numpy(), want_instance)
    assert out["instance_center"].shape == (n, 3) and out["bbox"].shape == (3, 6)
    assert np.abs(out["instance_center"].numpy() - want_center).max() <= 2.0 ** -22  # (fp32 roundings of means below 4)
    assert np.array_equal(out["bbox"].numpy(), want_bbox.astype(np.float32))
    assert (out["instance_center"].numpy()[ignored] == -1).all()
