"""Masked Scene Contrast v1m2 (CSC): the partitioned InfoNCE loss and one training step of the CSC config's model,
ao_amd/csrc/msc_csc.hip against AO_AMD_MSC=torch (the reference's eager statements on the same device).

    python tools/bench_msc_csc.py [--channels 96] [--rooms 8] [--points 40000] [--repeats 5] [--warmup 2] [--no-step]

csc_nce: forward + backward at --channels, t = 0.4, r1 = 0.125, r2 = 0.5 in rooms of 1.2 x 1.0 x 0.5 m, for one scene of 8192
pairs and for 8 scenes of 1024: time, and the allocator's peak over one call.  The step: --rooms synthetic rooms
(ao_amd.synth.room_cloud, --points each), each as two frames through the two transform lists of
configs/scannet/pretrain-msc-v1m2-0-spunet-csc.py (0.025 m grid) and pair_views, collated; the model is that config's (r1 = 2,
r2 = 20).  Median of --repeats after --warmup calls, the host clock around calls that end in a device synchronise.  One JSON
line per figure, printed and written to profiles/msc_csc_bench.jsonl; the last carries the build digest."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_msc import both  # noqa: E402


def recorded_config():
    with open(os.path.join(ROOT, "tests", "golden", "msc_csc_config.json")) as f:
        return json.load(f)


def loss_case(scenes, per_scene, c, g):
    """(f1, f2, origin1, origin2, offset, pairs): `scenes` rooms of per_scene + 100 points per view, per_scene pairs each"""
    import torch

    n = per_scene + 100
    f1 = torch.randn(scenes * n, c, device="cuda", generator=g).requires_grad_(True)
    f2 = (0.6 * f1.detach() + 0.4 * torch.randn(scenes * n, c, device="cuda", generator=g)).requires_grad_(True)
    extent = torch.tensor([1.2, 1.0, 0.5], device="cuda")
    o1 = torch.rand(scenes * n, 3, device="cuda", generator=g) * extent
    o2 = o1 + (torch.rand(scenes * n, 3, device="cuda", generator=g) - 0.5) * 0.008
    rows = torch.cat([s * n + torch.randperm(n, device="cuda", generator=g)[:per_scene] for s in range(scenes)])
    rows = rows[torch.randperm(rows.numel(), device="cuda", generator=g)]  # as the max_pair permutation leaves them
    offset = (torch.arange(1, scenes + 1, device="cuda") * n).int()
    return f1, f2, o1, o2, offset, torch.stack([rows, rows], 1)


def batch_of_rooms(rooms, points):
    import numpy as np
    import torch

    from ao_amd import synth
    from ao_amd.ptv2 import transform as T
    cfg = recorded_config()
    gens = dict(generator=torch.Generator().manual_seed(0), device_generator=torch.Generator(device="cuda").manual_seed(0))
    lists = [T.Compose(cfg[k], fuse=True, **gens) for k in ("view1_transform", "view2_transform")]
    out = []
    for room in range(rooms):
        rng = np.random.default_rng(room)
        coord = torch.from_numpy(synth.room_cloud(points, seed=room)).float().cuda()
        color = torch.from_numpy(rng.uniform(0, 255, (points, 3)).astype(np.float32)).cuda()
        frames = [dict(coord=coord.clone(), color=color.clone()) for _ in range(2)]
        out.append(T.pair_views(frames[0], frames[1], lists[0], lists[1]))
    return T.point_collate(out)


def main():
    ap = argparse.ArgumentParser()
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

    c = args.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    for scenes, per_scene in ((1, 8192), (8, 1024)):
        f1, f2, o1, o2, offset, pairs = loss_case(scenes, per_scene, c, g)

        def nce():
            f1.grad = f2.grad = None
            msc.csc_nce(f1, f2, o1, o2, offset, pairs, 0.4, 0.125, 0.5)[0].backward()

        emit(figure="csc_nce_fwd_bwd", scenes=scenes, pairs_per_scene=per_scene, channels=c, t=0.4, r1=0.125, r2=0.5,
             **both(nce, args.repeats, args.warmup))

    if not args.no_step:
        batch = batch_of_rooms(args.rooms, args.points)
        views = [batch[k] for k in ("view1_origin_coord", "view1_offset", "view2_origin_coord", "view2_offset")]
        os.environ["AO_AMD_MSC"] = "hip"
        emit(figure="batch", rooms=args.rooms, points_per_room=args.points, view1_points=batch["view1_coord"].shape[0],
             view2_points=batch["view2_coord"].shape[0], matched_rows=msc.match_pairs(*views, 8, 0.03, 1 << 30).shape[0])
        torch.manual_seed(0)
        model = msc.MaskedSceneContrastCSC(**{k: v for k, v in recorded_config()["model"].items() if k != "type"}).cuda().train()

        def step():
            model.zero_grad(set_to_none=True)
            model(dict(batch), mix=(False, False))["loss"].backward()

        emit(figure="train_step", config="pretrain-msc-v1m2-0-spunet-csc", **both(step, args.repeats, args.warmup))
    emit(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0), numpy=np.__version__,
         torch=torch.__version__)
    with open(os.path.join(ROOT, "profiles", "msc_csc_bench.jsonl"), "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
