#!/usr/bin/env python
"""Times SPVCNN's point-voxel map, its two operators at the levels and widths the model uses them, forward + backward, and one
training step of SPVCNN(6, 13), on ao_amd/csrc/spv_map.hip / spv_ops.hip against the eager statements (AO_AMD_SPVCNN=torch) on
the same device and the same map: warm-up, alternating runs, medians, allocator peaks above the inputs.

    python tools/bench_spvcnn.py [--points 100000] [--rounds 11] [--iters 10] [--skip-model]

The scene is the room of bench.py (ao_amd/synth.py: room_scene) on a 0.05 m grid, so that some voxels hold several points.
One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import spvcnn, synth  # noqa: E402

# (operator, level, C) as SPVCNN.forward calls them
CALLS = [("voxelize", 0, 6), ("devoxelize", 0, 32), ("voxelize", 0, 32), ("devoxelize", 4, 256), ("voxelize", 4, 256),
         ("devoxelize", 2, 128), ("voxelize", 2, 128), ("devoxelize", 0, 96)]


def timed(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def compare(step, rounds, iters, **row):
    ms, mem = {"hip": [], "torch": []}, {}
    for how in ms:   # warm-up and peak memory
        os.environ["AO_AMD_SPVCNN"] = how
        for _ in range(3):
            step()
        mem[how] = peak(step)
    for _ in range(rounds):   # alternating
        for how in ms:
            os.environ["AO_AMD_SPVCNN"] = how
            ms[how].append(timed(step, iters))
    med = {how: statistics.median(v) for how, v in ms.items()}
    print(json.dumps(dict(row, hip_ms=round(med["hip"], 4), torch_ms=round(med["torch"], 4), speedup=round(med["torch"] / med["hip"], 2),
                          hip_min_ms=round(min(ms["hip"]), 4), torch_min_ms=round(min(ms["torch"]), 4),
                          hip_peak_mb=round(mem["hip"] / 2 ** 20, 2), torch_peak_mb=round(mem["torch"] / 2 ** 20, 2), rounds=rounds,
                          iters=iters)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    pts = synth.room_scene(seed=0, room=1, point_max=args.points)
    coord = torch.from_numpy(np.floor((pts - pts.min(0)) / 0.05).astype(np.int32)).cuda()
    offset = torch.tensor([coord.shape[0]], dtype=torch.int32, device="cuda")
    pv = spvcnn.point_voxel_map(coord, offset)
    ms = statistics.median(timed(lambda: spvcnn.point_voxel_map(coord, offset), 3) for _ in range(args.rounds))
    print(json.dumps(dict(figure="map", points=pv.n, voxels=pv.n_vox, most_points=[int(pv.counts(l).max()) for l in range(5)],
                          map_and_tables_ms=round(ms, 3))), flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, level, C in CALLS:
        rows_in, rows_out = (pv.n_vox[level], pv.n) if name == "devoxelize" else (pv.n, pv.n_vox[level])
        x = torch.randn(rows_in, C, device="cuda", generator=g, requires_grad=True)
        go = torch.randn(rows_out, C, device="cuda", generator=g)
        add = torch.randn(pv.n, C, device="cuda", generator=g, requires_grad=True) if name == "devoxelize" and level else None

        def step():
            if name == "devoxelize":
                return torch.autograd.grad(spvcnn.devoxelize(x, pv, level, add=add), (x,) if add is None else (x, add), go)
            return torch.autograd.grad(spvcnn.voxelize(x, pv, level), x, go)

        compare(step, args.rounds, args.iters, figure=name, level=level, C=C, add=add is not None)
    if args.skip_model:
        return
    torch.manual_seed(0)
    model = spvcnn.SPVCNN(6, 13).cuda().train()
    data = dict(discrete_coord=coord, offset=offset, feat=torch.randn(pv.n, 6, device="cuda", generator=g))
    label = torch.randint(0, 13, (pv.n,), device="cuda", generator=g)

    def train_step():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(data), label).backward()

    compare(train_step, args.rounds, 3, figure="training step", model="SPVCNN(6, 13)", points=pv.n)


if __name__ == "__main__":
    main()
