"""PointGroup's clustering stage: ball query, clustering and proposals of ao_amd/csrc/pointgroup.hip on one synthetic scene of
ScanNet size, against AO_AMD_PG=torch.

    python tools/bench_pointgroup.py [--points 150000] [--blobs 40] [--spread 1 4] [--repeats 20] [--torch-repeats 3] [--warmup 2]

The scene: --points shifted points in voxel units (the model's (coord + bias_pred) / voxel_size).  70 % of them lie around
--blobs predicted centres (a Gaussian of --spread voxels per blob, drawn uniformly; 4 classes), the rest on the surfaces of a synthetic room
(ao_amd.synth.room_cloud at 0.02 m per voxel) with the ignored classes 0 and 1.  radius 1.5, min_points 50, propose_points 100
(configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py).  The clustered points are those of the classes 2..5.

Each stage is timed on both paths in alternation, warm, the host clock around calls that end in a device synchronise (every
stage ends in a read-back).  `capped_share` is the share of the clustered points with more than PG_BALL_CAP neighbours, counted
by an eager distance count.  The results of the two paths are compared at this size: the lists must be equal (a pair within
rounding of the radius may differ: their number is printed), point_cluster, masks and classes equal, scores to 1e-6.
One JSON line per figure; the last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def scene(points, blobs, spread, seed=0):
    import numpy as np

    from ao_amd import synth

    rng = np.random.default_rng(seed)
    n_obj = int(points * 0.7)
    room = synth.room_cloud(points - n_obj, seed=seed) / 0.02
    lo, hi = room.min(0), room.max(0)
    centres = rng.uniform(lo, hi, (blobs, 3))
    spread = rng.uniform(spread[0], spread[1], blobs)
    classes = rng.integers(2, 6, blobs)
    of = rng.integers(0, blobs, n_obj)
    obj = centres[of] + rng.normal(0.0, 1.0, (n_obj, 3)) * spread[of, None]
    coords = np.concatenate([obj, room]).astype(np.float32)
    label = np.concatenate([classes[of], rng.integers(0, 2, points - n_obj)]).astype(np.int64)
    perm = rng.permutation(points)
    return coords[perm], label[perm]


def timed(fn, repeats, warmup):
    import torch

    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(wall), 3), min_ms=round(min(wall), 3), max_ms=round(max(wall), 3), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--blobs", type=int, default=40)
    ap.add_argument("--spread", type=float, nargs=2, default=(1.0, 4.0))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib, pointgroup

    coords, label = scene(args.points, args.blobs, args.spread)
    keep = np.nonzero(label >= 2)[0]
    sub = torch.from_numpy(coords[keep]).cuda()
    sub_label = torch.from_numpy(label[keep]).int().cuda()
    offsets = torch.tensor([0, keep.shape[0]], dtype=torch.int32, device="cuda")
    n, radius = keep.shape[0], 1.5
    prob = torch.softmax(torch.randn(args.points, 20, device="cuda") + 4.0 * torch.nn.functional.one_hot(
        torch.from_numpy(label).cuda(), 20), -1)
    segment_pred = prob.max(1)[1]
    kept = torch.from_numpy(keep).cuda()

    def stages(path):
        os.environ["AO_AMD_PG"] = path
        idx, start_len, capped = pointgroup.ball_query(sub, offsets, radius)
        sub_cluster, sizes, firsts = pointgroup.cluster(sub_label, idx, start_len, 50, capped)
        point_cluster = torch.full((args.points,), -1, dtype=torch.int32, device="cuda")
        point_cluster[kept] = sub_cluster
        out = pointgroup.proposals(point_cluster, sizes, kept[firsts.long()].int(), segment_pred, prob, 100)
        return (idx, start_len, capped), (sub_cluster, sizes, firsts), point_cluster, out

    res = {path: stages(path) for path in ("hip", "torch")}
    (idx, start_len, capped), (sub_cluster, sizes, firsts), point_cluster, (scores, masks, classes) = res["hip"]
    (tidx, tstart_len, tcapped), (tsub, tsizes, _), _, (tscores, tmasks, tclasses) = res["torch"]
    # the capped share, counted by an eager distance count (the lists themselves stop at the cap)
    over = 0
    for at in range(0, n, 512):
        q = sub[at:at + 512]
        d = q[:, None, :] - sub[None, :, :]
        over += int((((d * d).sum(-1) < radius * radius).sum(1) > pointgroup.BALL_CAP).sum())
    lens = start_len[:, 1].long()
    print(json.dumps(dict(figure="scene", points=args.points, spread=list(args.spread), clustered=n, blobs=args.blobs, radius=radius, n_active=int(idx.numel()),
                          mean_len=round(float(lens.float().mean()), 1), max_len=int(lens.max()), capped=bool(capped),
                          capped_points=over, capped_share=round(over / n, 5), clusters=int(sizes.numel()),
                          proposals=int(scores.numel()))))
    same_lists = bool(torch.equal(start_len, tstart_len) and torch.equal(idx, tidx))
    print(json.dumps(dict(figure="parity", lists_equal=same_lists, differing_lens=int((start_len[:, 1] != tstart_len[:, 1]).sum()),
                          capped_equal=capped == tcapped, point_cluster_equal=bool(torch.equal(sub_cluster, tsub)),
                          masks_equal=bool(masks.shape == tmasks.shape and torch.equal(masks, tmasks)),
                          classes_equal=bool(classes.shape == tclasses.shape and torch.equal(classes, tclasses)),
                          score_max_diff=float((scores - tscores).abs().max()) if scores.shape == tscores.shape and scores.numel() else None)))

    def ball():
        pointgroup.ball_query(sub, offsets, radius)

    def clus():
        pointgroup.cluster(sub_label, idx, start_len, 50, capped)

    def prop():
        pointgroup.proposals(point_cluster, sizes, kept[firsts.long()].int(), segment_pred, prob, 100)

    def whole():
        stages(os.environ["AO_AMD_PG"])

    for name, fn in (("ball_query", ball), ("cluster", clus), ("proposals", prop), ("all_three", whole)):
        row = dict(figure=name)
        for path, repeats in (("hip", args.repeats), ("torch", args.torch_repeats), ("hip", args.repeats), ("torch", args.torch_repeats)):
            os.environ["AO_AMD_PG"] = path
            t = timed(fn, repeats, args.warmup)
            row[path] = t if path not in row else dict(row[path], again_ms=t["ms"])
        row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row))
    print(json.dumps(dict(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0),
                          numpy=np.__version__, torch=torch.__version__)))


if __name__ == "__main__":
    main()
