"""tests/golden/make_golden_tester.py -- tests/golden/tester.npz: what the reference's test-time path computes, produced by
RUNNING the reference's own Python, unmodified, on the CPU.  Nothing here is read at test time except the file it writes.

Executed from the reference tree (its root is the first argument, or $POINTCEPT_ROOT):
  * pointcept/datasets/transform.py   CenterShift, NormalizeColor, RandomScale, RandomFlip, RandomRotateTargetAngle, Compose
  * pointcept/datasets/s3dis.py       S3DISDataset.prepare_test_data, called on a stand-in `self` that carries the members
                                      S3DISDataset.__init__ builds for test_mode (the transforms of the config's test_cfg)
  * pointcept/engines/test.py:94-138, 203-214 and pointcept/utils/misc.py intersection_and_union: the vote, the prediction
    and the summary numbers for recorded per-fragment logits (the loop is restated here line by line on torch CPU tensors:
    test.py itself needs a GPU and the whole training stack to import; intersection_and_union is the reference's)
The `pointcept*` package objects are empty namespace stubs, as in make_golden_host.py; pointcept.utils.logger / .cache are
stubbed as well (s3dis.py imports them for its constructor only; the logger needs a package this container lacks).

numpy note, as make_golden_host.py: GridSample gets grid_size=np.float32(g) so that `coord / grid_size` is an fp32 division on
the fp32 S3DIS cloud.  After a rotation the reference's coord is float64 and so is that division; ao_amd rounds the rotated
coordinates to fp32 first.  The clouds are therefore filtered below: a point within 1e-3 of a voxel border (in cell units, in
any augmentation) is dropped, so that both roundings put every point in the same voxel.

Also measured here and printed (tests/test_tester_host.py states the result): the fp32 distance between two summation
orders of the same vote, which is the tolerance the host test allows the eager VoteTable against the fixture.

usage:  python tests/golden/make_golden_tester.py <reference root>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import tester_cases as TC  # noqa: E402


def load_reference(ref):
    for name, sub in (("pointcept", "pointcept"), ("pointcept.utils", "pointcept/utils"),
                      ("pointcept.datasets", "pointcept/datasets")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, sub)]
        sys.modules[name] = m
    logger = types.ModuleType("pointcept.utils.logger")
    logger.get_root_logger = lambda *a, **k: __import__("logging").getLogger("pointcept")
    sys.modules["pointcept.utils.logger"] = logger
    cache = types.ModuleType("pointcept.utils.cache")
    cache.shared_dict = lambda *a, **k: None
    sys.modules["pointcept.utils.cache"] = cache
    T = importlib.import_module("pointcept.datasets.transform")
    D = importlib.import_module("pointcept.datasets.s3dis")
    M = importlib.import_module("pointcept.utils.misc")
    for mod in (T, D, M):
        assert mod.__file__.startswith(ref), mod.__file__
    return T, D, M


def with_fp32_grid(cfg):
    cfg = dict(cfg)
    cfg["voxelize"] = dict(cfg["voxelize"], grid_size=np.float32(cfg["voxelize"]["grid_size"]))
    return cfg


def gen_transforms(T, out):
    room = TC.synthetic_room(240, seed=3)
    coord, color = room["coord"].numpy(), room["color"].numpy()
    normal = np.random.default_rng(4).normal(size=coord.shape).astype(np.float32)
    out["tf_coord"], out["tf_color"], out["tf_normal"] = coord, color, normal

    def run(tag, t):
        d = t(dict(coord=coord.copy(), color=color.copy(), normal=normal.copy()))
        for key in ("coord", "color", "normal"):
            out["tf_%s_%s" % (tag, key)] = d[key]

    run("centershift_z", T.CenterShift(apply_z=True))
    run("centershift", T.CenterShift(apply_z=False))
    run("normalizecolor", T.NormalizeColor())
    run("scale09", T.RandomScale(scale=[0.9, 0.9]))
    run("scale105", T.RandomScale(scale=[1.05, 1.05]))
    run("flip", T.RandomFlip(p=1))
    run("flip0", T.RandomFlip(p=0))
    for name, angle, axis, center in (("rot_z_half", 1 / 2, "z", [0, 0, 0]), ("rot_z_one", 1, "z", [0, 0, 0]),
                                      ("rot_z_threehalf", 3 / 2, "z", [0, 0, 0]), ("rot_x_third", 1 / 3, "x", None),
                                      ("rot_y_quarter", 1 / 4, "y", [0.5, -0.25, 1.0])):
        run(name, T.RandomRotateTargetAngle(angle=[angle], axis=axis, center=center, p=1))
    run("compose", T.Compose([dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor"),
                              dict(type="RandomScale", scale=[0.95, 0.95]), dict(type="RandomFlip", p=1)]))


def away_from_borders(T, data, cfg, base):
    """indices of the points that are further than 1e-3 cells from a voxel border in every augmentation"""
    d = T.Compose(base)({k: v.copy() for k, v in data.items()})
    keep = np.ones(d["coord"].shape[0], bool)
    for aug in cfg["aug_transform"]:
        a = T.Compose(aug)({k: v.copy() for k, v in d.items()})
        cell = a["coord"].astype(np.float64) / float(cfg["voxelize"]["grid_size"])
        # (a coordinate that is exactly 0 -- the lowest point after CenterShift(apply_z=True) -- is 0 in both roundings)
        keep &= ((np.abs(cell - np.round(cell)) > 1e-3) | (cell == 0)).all(1)
    return np.nonzero(keep)[0]


def gen_fragments(T, D, out, tag, cfg, base, seed, with_normal):
    room = TC.synthetic_room(3000, seed=seed, classes=13 if tag == "s3dis" else 20)
    data = dict(coord=room["coord"].numpy(), color=room["color"].numpy(), segment=room["segment"].numpy())
    if with_normal:
        nrm = np.random.default_rng(seed + 1).normal(size=data["coord"].shape)
        data["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    for _ in range(50):  # dropping points can move the bounding box that CenterShift reads: filter to a fixed point
        keep = away_from_borders(T, {k: v for k, v in data.items() if k != "segment"}, cfg, base)
        if keep.shape[0] == data["coord"].shape[0]:
            break
        data = {k: v[keep] for k, v in data.items()}
    assert away_from_borders(T, {k: v for k, v in data.items() if k != "segment"}, cfg, base).shape[0] == data["coord"].shape[0]
    n = data["coord"].shape[0]
    cfg32 = with_fp32_grid(cfg)
    self = types.SimpleNamespace(
        get_data=lambda idx: {k: v.copy() for k, v in data.items()}, get_data_name=lambda idx: tag,
        transform=T.Compose(base), test_voxelize=T.TRANSFORMS.build(cfg32["voxelize"]), test_crop=None,
        post_transform=T.Compose(cfg32["post_transform"]), aug_transform=[T.Compose(a) for a in cfg32["aug_transform"]])
    np.random.seed(seed)
    result = D.S3DISDataset.prepare_test_data(self, 0)
    assert result["name"] == tag and np.array_equal(result["segment"], data["segment"])
    frags = result["fragment_list"]
    # fragments per augmentation: count.max() of that augmentation's voxelisation
    per_aug, aug_coord, aug_normal = [], [], []
    base_d = T.Compose(base)({k: v.copy() for k, v in data.items() if k != "segment"})
    for aug in self.aug_transform:
        a = aug({k: v.copy() for k, v in base_d.items()})
        aug_coord.append(np.asarray(a["coord"], np.float32))
        if with_normal:
            aug_normal.append(np.asarray(a["normal"], np.float32))
        per_aug.append(len(self.test_voxelize({k: (v.copy() if hasattr(v, "copy") else v) for k, v in a.items()})))
    assert sum(per_aug) == len(frags)
    out[tag + "_coord"], out[tag + "_color"], out[tag + "_segment"] = data["coord"], data["color"], data["segment"]
    if with_normal:
        out[tag + "_normal"], out[tag + "_aug_normal"] = data["normal"], np.stack(aug_normal)  # (n_aug, n, 3)
    out[tag + "_base_color"] = np.asarray(base_d["color"], np.float32)
    out[tag + "_aug_coord"] = np.stack(aug_coord)
    out[tag + "_per_aug"] = np.asarray(per_aug)
    out[tag + "_sizes"] = np.asarray([f["index"].shape[0] for f in frags])
    out[tag + "_index"] = np.concatenate([f["index"].numpy() for f in frags]).astype(np.int32)
    print(tag, "points", n, "fragments per augmentation", per_aug)
    return n, frags


def gen_vote(M, out, tag, n, frags, k, seed):
    """recorded logits per fragment -> test.py:94-123 (torch CPU, fp32), :125-138 per scene, :203-214 over two scenes"""
    g = torch.Generator().manual_seed(seed)
    sets = [f["index"] for f in frags]
    segment = torch.from_numpy(out[tag + "_segment"])
    logits = []
    for idx in sets:  # a noisy classifier: the label's class leads most of the time
        x = torch.randn(idx.numel(), k, generator=g) * 2
        lab = segment[idx].clamp_min(0)
        x[torch.arange(idx.numel()), lab] += 3.0
        logits.append(torch.round(x * 4).clamp(-127, 127) / 4)  # multiples of 1/4: stored as int8, exact in fp32
    pred = torch.zeros((n, k))
    for idx_part, x in zip(sets, logits):
        pred_part = torch.nn.functional.softmax(x, -1)
        bs = 0
        for be in torch.tensor([idx_part.numel()]):
            pred[idx_part[bs:be], :] += pred_part[bs:be]
            bs = be
    votes = pred.clone()
    pred = pred.max(1)[1].data.cpu().numpy()
    # the same vote with the fragments in reverse order: the fp32 spread between two summation orders
    rev = torch.zeros((n, k))
    for idx_part, x in zip(sets[::-1], logits[::-1]):
        rev[idx_part, :] += torch.nn.functional.softmax(x, -1)
    spread = float((rev - votes).abs().max())
    v64 = TC.votes64(n, k, sets, logits)
    band_share = float((TC.margin(v64) < 1e-4).double().mean())
    print(tag, "vote: max |order A - order B| = %.3e (max vote %.3f); points with float64 margin < 1e-4: %.5f"
          % (spread, float(votes.max()), band_share))
    seg = out[tag + "_segment"]
    intersection, union, target = M.intersection_and_union(pred, seg, k, -1)
    mask = union != 0
    iou_class = intersection / (union + 1e-10)
    out[tag + "_vote_logits_q4"] = (torch.cat(logits) * 4).to(torch.int8).numpy()
    out[tag + "_votes"] = votes.numpy()
    out[tag + "_pred"] = pred
    out[tag + "_order_spread"] = np.float64(spread)
    out[tag + "_intersection"], out[tag + "_union"], out[tag + "_target"] = intersection, union, target
    out[tag + "_scene_iou"] = np.float64(np.mean(iou_class[mask]))
    out[tag + "_scene_acc"] = np.float64(sum(intersection) / (sum(target) + 1e-10))
    return intersection, union, target


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("POINTCEPT_ROOT", "")
    assert os.path.isdir(os.path.join(ref, "pointcept")), "usage: make_golden_tester.py <reference root>"
    T, D, M = load_reference(os.path.abspath(ref))
    out = {}
    gen_transforms(T, out)
    n, frags = gen_fragments(T, D, out, "s3dis", TC.s3dis_cfg([0, 7]), TC.S3DIS_BASE_TRANSFORM, seed=21, with_normal=False)
    a = gen_vote(M, out, "s3dis", n, frags, 13, seed=22)
    cfg = dict(TC.SCANNET_TEST_CFG, aug_transform=TC.SCANNET_TEST_CFG["aug_transform"][:2])
    n, frags = gen_fragments(T, D, out, "scannet", cfg, TC.S3DIS_BASE_TRANSFORM, seed=31, with_normal=True)
    # test.py:203-214 over two "scenes" (the S3DIS scene and the same scene with the prediction of its first half only)
    half = out["s3dis_pred"].copy()
    half[half.shape[0] // 2:] = 0
    b = M.intersection_and_union(half, out["s3dis_segment"], 13, -1)
    intersection, union, target = (np.sum([x, y], axis=0) for x, y in zip(a, b))
    iou_class, accuracy_class = intersection / (union + 1e-10), intersection / (target + 1e-10)
    out["sum_half_pred"] = half
    out["sum_iou_class"], out["sum_acc_class"] = iou_class, accuracy_class
    out["sum_mIoU"], out["sum_mAcc"] = np.float64(np.mean(iou_class)), np.float64(np.mean(accuracy_class))
    out["sum_allAcc"] = np.float64(sum(intersection) / (sum(target) + 1e-10))
    path = os.path.join(HERE, "tester.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
