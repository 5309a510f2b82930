"""Inputs and float64 statements shared by tests/test_tester_host.py, tests/test_gpu_tester.py and tools/bench_tester.py
(no test in here).  Everything is built on the CPU from a seed, so the host suite can check on its own what the GPU cases
assume about their inputs (the planted leading class, the guard band's share)."""
import numpy as np
import torch

S3DIS_TEST_CFG = dict(  # configs/s3dis/semseg-pt-v2m2-0-base.py:145-188 (values only)
    voxelize=dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="test", keys=("coord", "color"),
                  return_discrete_coord=True),
    crop=None,
    post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                    dict(type="Collect", keys=("coord", "discrete_coord", "index"), feat_keys=("coord", "color"))],
    aug_transform=[[dict(type="RandomScale", scale=[s, s])] for s in (0.9, 0.95, 1, 1.05, 1.1)]
    + [[dict(type="RandomScale", scale=[s, s]), dict(type="RandomFlip", p=1)] for s in (0.9, 0.95, 1, 1.05, 1.1)])
S3DIS_BASE_TRANSFORM = [dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")]

SCANNET_TEST_CFG = dict(  # configs/scannet/semseg-pt-v2m2-0-base.py:158-: the first four augmentations (rotations alone)
    voxelize=dict(type="GridSample", grid_size=0.02, hash_type="fnv", mode="test", keys=("coord", "color", "normal")),
    crop=None,
    post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                    dict(type="Collect", keys=("coord", "index"), feat_keys=("coord", "color", "normal"))],
    aug_transform=[[dict(type="RandomRotateTargetAngle", angle=[a], axis="z", center=[0, 0, 0], p=1)]
                   for a in (0, 1 / 2, 1, 3 / 2)])


def s3dis_cfg(augs):
    return dict(S3DIS_TEST_CFG, aug_transform=[S3DIS_TEST_CFG["aug_transform"][i] for i in augs])


def fragments(n_total, n, frags, seed):
    """`frags` index sets of n distinct points each out of n_total (n <= n_total), in random order"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n_total, generator=g)[:n] for _ in range(frags)]


def spread_logits(n, c, seed, spread=60.0):
    """rows over the whole +-spread range: saturated softmax outputs, exp underflow and near ties in one input"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, c, generator=g) * 2 - 1) * spread
    x[::3] = x[::3] / 30  # a third of the rows with a flat distribution
    return x


def planted(n_total, c, frags, seed, lead=12.0):
    """(index sets, logits, leader): every point is in two thirds of the fragments and its leading class gets +lead in each,
    so the float64 top-two vote margin is >= 1 wherever a point was visited (share of near ties: 0)"""
    g = torch.Generator().manual_seed(seed)
    leader = torch.randint(0, c, (n_total,), generator=g)
    sets, logits = [], []
    for f in range(frags):
        keep = torch.nonzero((torch.arange(n_total) + f) % 3 != 0).reshape(-1)
        keep = keep[torch.randperm(keep.numel(), generator=g)]
        x = torch.randn(keep.numel(), c, generator=g) * 2
        x[torch.arange(keep.numel()), leader[keep]] += lead
        sets.append(keep)
        logits.append(x)
    return sets, logits, leader


def votes64(n_total, c, sets, logits):
    """the float64 statement: softmax in float64 of the logits as given (bf16 / fp32 values widened exactly), float64 sums"""
    v = torch.zeros(n_total, c, dtype=torch.float64)
    for idx, x in zip(sets, logits):
        v[idx.long().cpu()] += torch.softmax(x.detach().cpu().double(), -1)
    return v


def margin(v):
    """top-two margin of every row"""
    top = torch.topk(v, 2, dim=1)[0]
    return top[:, 0] - top[:, 1]


def literal_loop(model, fragment_list, n_points, num_classes, device, collate, dtype=torch.float32):
    """pointcept/engines/test.py:94-123 written out (fragment batch 1), the table in `dtype`; also every fragment's logits"""
    pred = torch.zeros((n_points, num_classes), dtype=dtype, device=device)
    kept = []
    for i in range(len(fragment_list)):
        input_dict = collate(fragment_list[i:i + 1])
        for key in input_dict.keys():
            if isinstance(input_dict[key], torch.Tensor):
                input_dict[key] = input_dict[key].to(device, non_blocking=True)
        idx_part = input_dict["index"]
        with torch.no_grad():
            pred_part = model(input_dict)["seg_logits"]
            kept.append((idx_part, pred_part))
            pred_part = torch.nn.functional.softmax(pred_part.to(dtype), -1)
        bs = 0
        for be in input_dict["offset"]:
            pred[idx_part[bs:be], :] += pred_part[bs:be]
            bs = be
    return pred, kept


def synthetic_room(n, seed, classes=13):
    """coord (n, 3) fp32 with several points per 4 cm voxel, color (n, 3) in [0, 255], segment (n,) with ignored points"""
    from tests import synth

    rng = np.random.default_rng(seed)
    base = synth.room_cloud(n // 3, seed=seed)
    pts = np.concatenate([base + rng.normal(0, 0.012, base.shape).astype(np.float32) for _ in range(3)])
    pts = np.ascontiguousarray(pts[rng.permutation(pts.shape[0])], dtype=np.float32)
    color = rng.integers(0, 256, size=pts.shape).astype(np.float32)
    segment = rng.integers(-1, classes, size=pts.shape[0]).astype(np.int64)
    return dict(coord=torch.from_numpy(pts), color=torch.from_numpy(color), segment=torch.from_numpy(segment), name="room")
