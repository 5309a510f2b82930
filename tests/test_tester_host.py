"""CPU: ao_amd/ptv2/tester.py (VoteTable's eager path, test_scene, SemSegTester's bookkeeping), the test-time transforms of
ao_amd/ptv2/transform.py and `registry.register(TEST=...)` against tests/golden/tester.npz, which the reference's own code
produced (tests/golden/make_golden_tester.py).

Tolerances.  Votes: the generator measures the fp32 distance between two summation orders of the fixture's vote (fragments in
list order against reverse order): 1.9e-6 at a largest vote of 9.5; it is stored as `s3dis_order_spread` and is the tolerance
here (the eager path keeps the reference's order, so it is in fact met with 0).  Prediction: equal wherever the float64
top-two margin is at least twice that spread; at most 0.5 % of the points may fall below (measured by the generator with a
50 x wider band, 1e-4: 0.034 %).  Rotations: the reference's output is float64, this module's is that value rounded to fp32
once: half an ulp of a coordinate below 16 m is 4.8e-7, bound 1e-6.  Everything else in the transforms is bitwise.  Summary
numbers: 1e-12.
"""
import ctypes
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import tester_cases as TC
from tests.conftest import GOLDEN, ROOT
from tests.test_registry_host import Registry

CAP = 0.005


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "tester.npz"), allow_pickle=False)


def _vote_inputs(z):
    sizes = z["s3dis_sizes"]
    sets = [torch.from_numpy(a.astype(np.int64)) for a in np.split(z["s3dis_index"], np.cumsum(sizes)[:-1])]
    logits = torch.from_numpy(z["s3dis_vote_logits_q4"].astype(np.float32) / 4)
    return sets, list(torch.split(logits, [int(s) for s in sizes]))


def check_transforms(z, device):
    """every new transform against the reference's output on the fixture's cloud (shared with tests/test_gpu_tester.py)"""
    from ao_amd.ptv2 import transform as T

    def data():
        return {k: torch.from_numpy(z["tf_" + k]).to(device) for k in ("coord", "color", "normal")}

    def same(tag, got, atol=None):
        for key in ("coord", "color", "normal"):
            want = z["tf_%s_%s" % (tag, key)]
            have = got[key].cpu().numpy()
            assert have.dtype == np.float32, (tag, key, have.dtype)
            if atol is None or want.dtype == np.float32:
                assert np.array_equal(have, want.astype(np.float32)), (tag, key, np.abs(have - want).max())
            else:
                assert np.abs(have.astype(np.float64) - want).max() <= atol, (tag, key, np.abs(have - want).max())

    same("centershift_z", T.CenterShift(apply_z=True)(data()))
    same("centershift", T.CenterShift(apply_z=False)(data()))
    same("normalizecolor", T.NormalizeColor()(data()))
    same("scale09", T.RandomScale(scale=[0.9, 0.9])(data()))
    same("scale105", T.RandomScale(scale=[1.05, 1.05])(data()))
    same("flip", T.RandomFlip(p=1)(data()))
    same("flip0", T.RandomFlip(p=0)(data()))
    for name, angle, axis, center in (("rot_z_half", 1 / 2, "z", [0, 0, 0]), ("rot_z_one", 1, "z", [0, 0, 0]),
                                      ("rot_z_threehalf", 3 / 2, "z", [0, 0, 0]), ("rot_x_third", 1 / 3, "x", None),
                                      ("rot_y_quarter", 1 / 4, "y", [0.5, -0.25, 1.0])):
        same(name, T.RandomRotateTargetAngle(angle=[angle], axis=axis, center=center, p=1)(data()), atol=1e-6)
    same("compose", T.Compose([dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor"),
                               dict(type="RandomScale", scale=[0.95, 0.95]), dict(type="RandomFlip", p=1)])(data()))
    # draws come from a generator: two runs with equal seeds agree, a non-degenerate range stays inside it
    a = T.RandomScale(scale=[0.9, 1.1], anisotropic=True)(data(), generator=torch.Generator().manual_seed(3))["coord"]
    b = T.RandomScale(scale=[0.9, 1.1], anisotropic=True)(data(), generator=torch.Generator().manual_seed(3))["coord"]
    assert torch.equal(a, b)
    ratio = (a / data()["coord"]).cpu()
    assert float(ratio.min()) >= 0.9 - 1e-6 and float(ratio.max()) <= 1.1 + 1e-6
    assert T.ToTensor()(data())["coord"].dtype == torch.float32 and T.ToTensor()("name") == "name"
    with pytest.raises(KeyError):
        T.Compose([dict(type="ElasticDistortion")])


def test_transforms_against_the_fixture(z):
    check_transforms(z, "cpu")


def test_eager_vote_table_against_the_fixture(z):
    from ao_amd.ptv2 import VoteTable

    sets, logits = _vote_inputs(z)
    n, k = z["s3dis_votes"].shape
    tol = float(z["s3dis_order_spread"])
    assert 0 < tol < 4e-6
    one = VoteTable(n, k, "cpu")
    for idx, x in zip(sets, logits):
        one.add(x, idx, check=True)
    ends = torch.tensor([s.numel() for s in sets]).cumsum(0).int()
    batched = VoteTable(n, k, "cpu").add(torch.cat(logits), torch.cat(sets).int(), ends)
    want = torch.from_numpy(z["s3dis_votes"])
    for t in (one, batched):
        assert t.votes.dtype == torch.float32
        assert float((t.votes - want).abs().max()) <= tol
    assert torch.equal(one.votes, batched.votes)
    m = TC.margin(TC.votes64(n, k, sets, logits))
    keep = m >= 2 * tol
    assert 1.0 - float(keep.double().mean()) <= CAP
    pred = one.predict()
    assert pred.dtype == torch.int64
    assert torch.equal(pred[keep], torch.from_numpy(z["s3dis_pred"]).long()[keep])
    with pytest.raises(ValueError, match="twice"):
        VoteTable(n, k, "cpu").add(logits[0], torch.cat([sets[0][:-1], sets[0][:1]]), check=True)
    with pytest.raises(IndexError):
        VoteTable(n, k, "cpu").add(logits[0], sets[0] + n, check=True)
    with pytest.raises(ValueError):
        VoteTable(n, k, "cpu").add(logits[0][:, :5], sets[0])


@pytest.mark.parametrize("c", [2, 13, 20, 32, 33, 200, 256])
def test_planted_inputs_have_no_near_ties(c):
    """what tests/test_gpu_tester.py assumes of its synthetic logits: every point visited, float64 margin >= 1, leader wins"""
    sets, logits, leader = TC.planted(20000, c, 12, seed=c)
    v = TC.votes64(20000, c, sets, logits)
    assert float(TC.margin(v).min()) >= 1.0
    assert torch.equal(v.max(1)[1], leader)
    assert all(torch.unique(s).numel() == s.numel() for s in sets)


class _Recorded(torch.nn.Module):
    """a model stand-in: returns the fixture's logits for the rows it is given (looked up through `index`)"""

    def __init__(self, sets, logits, n, k):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0
        self.by_frag = {s.numpy().tobytes(): x for s, x in zip(sets, logits)}
        assert len(self.by_frag) == len(sets)

    def forward(self, input_dict):
        self.calls += 1
        out, start = [], 0
        for end in input_dict["offset"].tolist():
            s = input_dict["index"][start:end]
            out.append(self.by_frag[s.long().numpy().tobytes()])
            start = end
        return dict(seg_logits=torch.cat(out))


def _cfg(path, k, dataset_type="S3DISDataset"):
    return types.SimpleNamespace(save_path=str(path), test_epoch=3, dataset_type=dataset_type, empty_cache=False,
                                 data=types.SimpleNamespace(num_classes=k, ignore_index=-1, names=["c%d" % i for i in range(k)]))


class _Loader(list):
    batch_size = 1
    dataset = None


def _scene(z, sets, name="s3dis"):
    frags = [dict(coord=torch.zeros(s.numel(), 3), index=s, offset=torch.tensor([s.numel()])) for s in sets]
    return [dict(fragment_list=frags, segment=z["s3dis_segment"], name=name)]


@pytest.mark.parametrize("fragment_batch", [1, 4])
def test_tester_runs_a_scene_and_then_resumes_from_its_file(z, tmp_path, fragment_batch, caplog):
    from ao_amd.ptv2 import SemSegTester

    sets, logits = _vote_inputs(z)
    n, k = z["s3dis_votes"].shape
    model = _Recorded(sets, logits, n, k)
    tester = SemSegTester(fragment_batch=fragment_batch)
    assert tester.collate_fn([1, 2]) == [1, 2]
    with caplog.at_level(logging.INFO, logger="pointcept"):
        result = tester(_cfg(tmp_path, k), _Loader([_scene(z, sets)]), model)
    assert model.calls == -(-len(sets) // fragment_batch) and not model.training
    path = os.path.join(str(tmp_path), "result", "test_epoch3", "s3dis_pred.npy")
    pred = np.load(path)
    tol = float(z["s3dis_order_spread"])
    keep = (TC.margin(TC.votes64(n, k, sets, logits)) >= 2 * tol).numpy()
    assert np.array_equal(pred[keep], z["s3dis_pred"][keep])
    if np.array_equal(pred, z["s3dis_pred"]):
        inter, union, target = z["s3dis_intersection"], z["s3dis_union"], z["s3dis_target"]
        assert abs(result["mIoU"] - np.mean(inter / (union + 1e-10))) <= 1e-12
        line = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Test: s3dis [1/1]")]
        assert len(line) == 1
        acc, iou = re.search(r"Accuracy (\S+) \(", line[0]).group(1), re.search(r"mIoU (\S+) \(", line[0]).group(1)
        assert acc == "%.4f" % float(z["s3dis_scene_acc"]) and iou == "%.4f" % float(z["s3dis_scene_iou"])
    assert any("Val result: mIoU/mAcc/allAcc" in r.getMessage() for r in caplog.records)

    class Raises(torch.nn.Module):
        def forward(self, input_dict):
            raise AssertionError("the resume path must not run the network")

    again = tester(_cfg(tmp_path, k), _Loader([_scene(z, sets)]), Raises())
    assert again["mIoU"] == result["mIoU"] and np.array_equal(again["iou_class"], result["iou_class"])


def test_summary_numbers_against_the_fixture(z, tmp_path):
    """two scenes loaded from their files: test.py:125-138 per scene, :203-214 over both"""
    from ao_amd.ptv2 import SemSegTester
    from ao_amd.ptv2.tester import _counts_numpy

    k = 13
    c = _counts_numpy(z["s3dis_pred"], z["s3dis_segment"], k, -1)
    assert np.array_equal(c[0], z["s3dis_intersection"]) and np.array_equal(c[2], z["s3dis_target"])
    assert np.array_equal(c[1] + c[2] - c[0], z["s3dis_union"])
    out = os.path.join(str(tmp_path), "result", "test_epoch3")
    os.makedirs(out)
    np.save(os.path.join(out, "a_pred.npy"), z["s3dis_pred"])
    np.save(os.path.join(out, "b_pred.npy"), z["sum_half_pred"])
    sets, _ = _vote_inputs(z)
    loader = _Loader([_scene(z, sets, "a"), _scene(z, sets, "b")])
    result = SemSegTester()(_cfg(tmp_path, k), loader, torch.nn.Linear(1, 1))
    assert np.abs(result["iou_class"] - z["sum_iou_class"]).max() <= 1e-12
    assert np.abs(result["acc_class"] - z["sum_acc_class"]).max() <= 1e-12
    for key in ("mIoU", "mAcc", "allAcc"):
        assert abs(result[key] - float(z["sum_" + key])) <= 1e-12, key


def test_scannet_submit_file_and_unsupported_datasets(z, tmp_path):
    from ao_amd.ptv2 import SemSegTester

    k = 13
    out = os.path.join(str(tmp_path), "result", "test_epoch3")
    os.makedirs(out)
    np.save(os.path.join(out, "scene0000_00_pred.npy"), z["s3dis_pred"])
    sets, _ = _vote_inputs(z)
    loader = _Loader([_scene(z, sets, "scene0000_00")])
    class2id = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14])
    loader.dataset = types.SimpleNamespace(class2id=class2id)
    SemSegTester()(_cfg(tmp_path, k, "ScanNetDataset"), loader, torch.nn.Linear(1, 1))
    got = np.loadtxt(os.path.join(out, "submit", "scene0000_00.txt"), dtype=np.int64)
    assert np.array_equal(got, class2id[z["s3dis_pred"]])
    text = open(os.path.join(out, "submit", "scene0000_00.txt")).read().split("\n")
    assert text[0] == str(class2id[z["s3dis_pred"][0]]) and len(text) == z["s3dis_pred"].shape[0] + 1
    for kind in ("SemanticKITTIDataset", "NuScenesDataset"):
        with pytest.raises(NotImplementedError, match="SemanticKITTIDataset and NuScenesDataset"):
            SemSegTester()(_cfg(tmp_path, k, kind), loader, torch.nn.Linear(1, 1))


def test_register_files_the_tester_under_the_reference_name():
    from ao_amd.ptv2 import SemSegTester, registry

    TEST, MODELS, OPTIMIZERS, LOSSES = Registry("test"), Registry("models"), Registry("optimizers"), Registry("losses")
    # without TEST the returned list is what it was
    assert registry.register(MODELS=MODELS, OPTIMIZERS=OPTIMIZERS) == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image",
                                                                      "FlatAdamW"]
    assert registry.register(MODELS=MODELS, OPTIMIZERS=OPTIMIZERS, LOSSES=LOSSES)[-1] == "LovaszLoss"
    assert registry.register() == []
    done = registry.register(MODELS=MODELS, TEST=TEST)
    assert done == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image", "SemSegTester"]
    tester = TEST.build(dict(type="SemSegTester"))  # engines/test.py's `TEST.build(cfg.test)`
    assert isinstance(tester, SemSegTester) and tester.fragment_batch >= 1
    registry.register(TEST=TEST)  # a second registration replaces the entry
    with pytest.raises(KeyError):
        registry.register(TEST=TEST, force=False)


def test_vote_symbols_are_exported_with_their_arity():
    from ao_amd import _lib

    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptv2_hip.h")).read(), flags=re.S)
    for name, arity in (("seg_vote_add_hip_launcher", 10), ("seg_vote_status_hip_launcher", 2),
                        ("seg_vote_argmax_hip_launcher", 5)):
        assert hasattr(handle, name), name
        assert len(_lib._SIGNATURES[name][1]) == arity
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header).group(1)
        assert params.count(",") + 1 == arity
    L = _lib.lib()
    assert L.ptv2_abi_version() == 11
    # argument checks happen before anything is enqueued: no GPU needed to see them
    assert L.seg_vote_add_hip_launcher(5, 1, None, 0, None, 1, None, 10, None, None) == 1
    assert L.seg_vote_add_hip_launcher(5, 13, None, 0, None, 1, None, 10, None, None) == 1
    assert L.seg_vote_argmax_hip_launcher(-1, 13, None, None, None) == 1
    assert L.seg_vote_argmax_hip_launcher(0, 13, None, None, None) == 0
    assert L.seg_vote_status_hip_launcher(None, None) == 1
