"""The instance evaluator's association (ao_amd/pointgroup/evaluate.py on ao_amd/csrc/inseval.hip) on one
synthetic scene of ScanNet size, on three paths: HIP, AO_AMD_INSEVAL=torch, and the host loops of tests/inseval_ref.py (the
reference's own arithmetic) fed CPU masks.

    python tools/bench_inseval.py [--points 150000] [--origin 240000] [--proposals 100] [--instances 60] [--repeats 20]
                                  [--torch-repeats 5] [--host-repeats 3] [--warmup 2] [--out profiles/inseval_bench.jsonl]

The scene: --origin points on the surfaces of a synthetic room (ao_amd.synth.room_scene at 2 cm), --points of them kept as the sampled
cloud, nn_idx from pointops.knn_query(1, ...) as the evaluator takes it.  --instances ground-truth instances are the cells of
as many centres (20 classes, two of them ignored, 5 % of the points without instance); --proposals proposals each cover 90 % of
the sampled points of one instance plus 1 % of the others.

The device paths are timed warm and in alternation, the host clock around `associate` (it ends in a read-back); the host path
is the download of the masks (timed on its own), the reference's gather `pred_masks[:, idx]` and the loops.  `kernel` is the
launcher alone, ten calls between two events and their mean (each call also zeroes its three small outputs), against P * M * 4 bytes of mask reads at the HBM
rates of MI355X_MICROARCH.md: 8.0 TB/s peak, 6.29 TB/s measured for a float4 copy.  No time is a pass condition; the three
records must be equal.  One JSON line per figure, printed and written to --out; the last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def scene(args):
    import numpy as np
    import torch

    from ao_amd import pointops, synth

    rng = np.random.default_rng(0)
    room = synth.room_scene(seed=0, room=0, point_max=args.origin, density=20000.0, voxel=0.02)
    assert room.shape[0] == args.origin, (room.shape, args.origin)
    origin = torch.from_numpy(room).cuda()
    keep = np.sort(rng.choice(args.origin, args.points, replace=False))
    coord = origin[torch.from_numpy(keep).cuda()].contiguous()
    nn_idx, _ = pointops.knn_query(1, coord, torch.tensor([args.points], dtype=torch.int32, device="cuda"), origin,
                                   torch.tensor([args.origin], dtype=torch.int32, device="cuda"))
    nn_idx = nn_idx.reshape(-1).int()
    centres = origin[torch.from_numpy(rng.choice(args.origin, args.instances, replace=False)).cuda()]
    cell = torch.cdist(origin, centres).argmin(1).cpu().numpy()
    classes = rng.integers(0, 20, args.instances)
    instance = (cell * 7 + 3).astype(np.int64)
    segment = classes[cell].astype(np.int64)
    instance[rng.uniform(size=args.origin) < 0.05] = -1
    sampled_cell = cell[keep]
    masks = np.zeros((args.proposals, args.points), np.int32)
    of = rng.integers(0, args.instances, args.proposals)
    for row in range(args.proposals):
        inside = sampled_cell == of[row]
        masks[row] = np.where(inside, rng.uniform(size=args.points) < 0.9, rng.uniform(size=args.points) < 0.01)
    return dict(masks=torch.from_numpy(masks).cuda(), scores=torch.from_numpy(rng.uniform(size=args.proposals).astype(np.float32)),
                classes=torch.from_numpy(classes[of].astype(np.int64)), nn_idx=nn_idx, segment=torch.from_numpy(segment).cuda(),
                instance=torch.from_numpy(instance).cuda())


def timed(fn, repeats, warmup, sync):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(wall), 3), min_ms=round(min(wall), 3), max_ms=round(max(wall), 3), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--origin", type=int, default=240000)
    ap.add_argument("--proposals", type=int, default=100)
    ap.add_argument("--instances", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inseval_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib
    from ao_amd.pointgroup import evaluate
    from tests import inseval_ref

    ignore = (-1, 0, 1)
    s = scene(args)
    pred = dict(pred_masks=s["masks"], pred_scores=s["scores"], pred_classes=s["classes"])
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def device(path):
        os.environ["AO_AMD_INSEVAL"] = path
        return evaluate.associate(pred, s["segment"], s["instance"], 20, ignore, -1, 100, s["nn_idx"])

    cpu = {}

    def download():
        cpu["masks"] = s["masks"].cpu()

    download()
    idx = s["nn_idx"].cpu().flatten().long()
    segment, instance = s["segment"].cpu().numpy(), s["instance"].cpu().numpy()

    def host():
        gathered = cpu["masks"][:, idx]  # the reference's host gather
        return inseval_ref.associate(gathered.numpy(), s["scores"].numpy(), s["classes"].numpy(), segment, instance, ignore, -1, 100)

    hip, eager, loops = device("hip"), device("torch"), host()
    equal = all(np.array_equal(getattr(hip, k), getattr(eager, k)) and np.array_equal(getattr(hip, k), loops[k]) for k in hip._fields)
    emit(figure="scene", points=args.points, origin=args.origin, proposals=args.proposals, instances=args.instances,
         gt_kept=int(hip.gt_instance_id.shape[0]), proposals_kept=int(hip.pred_row.shape[0]),
         mean_proposal_share=round(float(hip.pred_vert_count.mean()) / args.origin, 4), matches=int((hip.inter > 0).sum()))
    emit(figure="parity", records_equal=bool(equal))

    row = dict(figure="associate")
    sync = torch.cuda.synchronize
    for path, repeats in (("hip", args.repeats), ("torch", args.torch_repeats), ("hip", args.repeats), ("torch", args.torch_repeats)):
        t = timed(lambda: device(path), repeats, args.warmup, sync)
        row[path] = t if path not in row else dict(row[path], again_ms=t["ms"])
    row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
    emit(**row)
    emit(figure="host", download=timed(download, args.host_repeats, 1, sync), gather_and_loops=timed(host, args.host_repeats, 0, lambda: None))

    # the launcher alone: codes prepared once, one window
    ids, _, _, col, void = evaluate.gt_table(s["segment"], s["instance"], ignore, -1)
    g = int(ids.numel())
    assert g <= evaluate.BINS
    code = ((col + 1) * 2 + void.long()).int().contiguous()
    p, m = s["masks"].shape
    inter = torch.empty((p, g), dtype=torch.int32, device="cuda")
    vert, void_inter = torch.empty(p, dtype=torch.int32, device="cuda"), torch.empty(p, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def launch(nn):
        _lib.check(L.inseval_associate_hip_launcher(p, m, nn.numel() if nn is not None else m, g, s["masks"].data_ptr(), _lib.ptr(nn),
                                                    code.data_ptr(), inter.data_ptr(), vert.data_ptr(), void_inter.data_ptr(),
                                                    _lib.stream_ptr()), "inseval_associate_hip_launcher")

    for name, nn, pts in (("kernel_nn_idx", s["nn_idx"], args.origin), ("kernel_identity", None, args.points)):
        if nn is None:
            code = code[:m].contiguous()  # (any codes do: the time is the masks')
        for _ in range(3):
            launch(nn)
        us = []
        for _ in range(args.repeats):  # ten launches between two events: the launch latency of the first is shared
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                launch(nn)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e2)
        t = statistics.median(us)
        mask_bytes = p * m * 4
        emit(figure=name, us=round(t, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), repeats=args.repeats, points=pts,
             mask_bytes=mask_bytes, tb_per_s=round(mask_bytes / t / 1e6, 3), share_of_hbm_peak=round(mask_bytes / (t * 1e-6) / HBM_PEAK, 3),
             share_of_hbm_copy=round(mask_bytes / (t * 1e-6) / HBM_COPY, 3))
    emit(figure="build", info=L.ptv2_build_info().decode(), device=torch.cuda.get_device_name(0), numpy=np.__version__,
         torch=torch.__version__)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
