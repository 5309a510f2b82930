"""Masked Scene Contrast: the InfoNCE loss, the pair matching, the cross masks and one training step of the base config's model,
ao_amd/csrc/msc.hip against AO_AMD_MSC=torch (the reference's eager statements on the same device).

    python tools/bench_msc.py [--pairs 8192] [--channels 96] [--rooms 8] [--points 40000] [--repeats 5] [--warmup 2] [--no-step]

info_nce: forward + backward at --pairs, --channels for t = 0.4 and t = 0.07: time, the allocator's peak over one call, and the
share of the 157.3 TFLOP/s fp32 matrix rate counted on 2 M^2 C flops per product (one product forward, three backward).
match_pairs, cross_masks and the step: --rooms synthetic rooms (ao_amd.synth.room_cloud, --points each) through the transform
list of configs/scannet/pretrain-msc-v1m1-0-spunet-base.py (0.02 m grid, 0.6 sphere crop) and point_collate; the model is that
config's, view mixing off.  Median of --repeats after --warmup calls, the host clock around calls that end in a device
synchronise.  One JSON line per figure, printed and written to profiles/msc_bench.jsonl; the last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX = 157.3e12


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
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return dict(ms=round(statistics.median(wall), 3), min_ms=round(min(wall), 3), max_ms=round(max(wall), 3), repeats=repeats,
                peak_mb=round(peak / 2 ** 20, 1))


def both(fn, repeats, warmup):
    row = {}
    for path in ("hip", "torch"):
        os.environ["AO_AMD_MSC"] = path
        row[path] = timed(fn, repeats, warmup)
    row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
    return row


def recorded_configs():
    """the model and transform settings of the reference's two MSC configs, as recorded in tests/golden/msc_configs.json"""
    with open(os.path.join(ROOT, "tests", "golden", "msc_configs.json")) as f:
        return json.load(f)


def batch_of_rooms(rooms, points):
    import numpy as np
    import torch

    from ao_amd import synth
    from ao_amd.ptv2 import transform as T
    pipe = T.Compose(recorded_configs()["base"]["transform"], fuse=True, generator=torch.Generator().manual_seed(0),
                     device_generator=torch.Generator(device="cuda").manual_seed(0))
    out = []
    for room in range(rooms):
        rng = np.random.default_rng(room)
        normal = rng.normal(0, 1, (points, 3))
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        out.append(pipe(dict(coord=torch.from_numpy(synth.room_cloud(points, seed=room)).float().cuda(),
                             color=torch.from_numpy(rng.uniform(0, 255, (points, 3)).astype(np.float32)).cuda(),
                             normal=torch.from_numpy(normal.astype(np.float32)).cuda())))
    return T.point_collate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--channels", type=int, default=96)
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib, msc

    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    m, c = args.pairs, args.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    f1 = torch.randn(m + 1000, c, device="cuda", generator=g).requires_grad_(True)
    f2 = (0.6 * f1.detach() + 0.4 * torch.randn(m + 1000, c, device="cuda", generator=g)).requires_grad_(True)
    pairs = torch.stack([torch.randperm(m + 1000, device="cuda", generator=g)[:m]] * 2, 1)
    for t in (0.4, 0.07):
        def nce():
            f1.grad = f2.grad = None
            msc.info_nce(f1, f2, pairs, t)[0].backward()

        row = both(nce, args.repeats, args.warmup)
        flops = 4 * 2.0 * m * m * c  # one product forward; S again, P B and P^T A backward
        row["hip"]["share_of_fp32_matrix_peak"] = round(flops / (row["hip"]["ms"] * 1e-3) / PEAK_FP32_MATRIX, 4)
        emit(figure="info_nce_fwd_bwd", pairs=m, channels=c, t=t, **row)

    batch = batch_of_rooms(args.rooms, args.points)
    n1, n2 = batch["view1_coord"].shape[0], batch["view2_coord"].shape[0]
    views = [batch[k] for k in ("view1_origin_coord", "view1_offset", "view2_origin_coord", "view2_offset")]
    os.environ["AO_AMD_MSC"] = "hip"
    found = msc.match_pairs(*views, 8, 0.03, 1 << 30).shape[0]
    emit(figure="batch", rooms=args.rooms, points_per_room=args.points, view1_points=n1, view2_points=n2, matched_rows=found,
         patches=int(torch.unique(msc.patch_ids(*views, 0.1)).numel()))
    gen = torch.Generator(device="cuda").manual_seed(1)
    emit(figure="match_pairs", max_k=8, max_radius=0.03, max_pair=8192,
         **both(lambda: msc.match_pairs(*views, 8, 0.03, 8192, generator=gen), args.repeats, args.warmup))
    emit(figure="cross_masks", mask_grid_size=0.1, mask_rate=0.4,
         **both(lambda: msc.cross_masks(*views, 0.1, 0.4), args.repeats, args.warmup))

    if not args.no_step:
        torch.manual_seed(0)
        model = msc.MaskedSceneContrast(**{k: v for k, v in recorded_configs()["base"]["model"].items() if k != "type"}).cuda().train()

        def step():
            model.zero_grad(set_to_none=True)
            model(dict(batch), mix=(False, False))["loss"].backward()

        emit(figure="train_step", config="pretrain-msc-v1m1-0-spunet-base", mixing=False, **both(step, args.repeats, args.warmup))
    emit(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0), numpy=np.__version__,
         torch=torch.__version__)
    with open(os.path.join(ROOT, "profiles", "msc_bench.jsonl"), "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
