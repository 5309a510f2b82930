#!/usr/bin/env python
"""Times one OctFormerBlock's attention and CPE operators, forward + backward, on ao_amd/csrc/oct_attention.hip and
oct_dwconv.hip against the eager statements (AO_AMD_OCTFORMER=torch) on the same device: warm-up, alternating runs, medians,
peak memory above the inputs and the device launches of one forward + backward.

    python tools/bench_octformer.py [--rounds 15] [--iters 10]

One JSON line per (n, C, H, D)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import octformer  # noqa: E402

SIZES = [(40000, 96, 6), (10000, 192, 12), (2500, 384, 24)]
K = 26


def scene(n, clouds=2, depth=9, seed=0):
    """n unique voxels per the whole batch, drawn on a surface-like slab so that neighbours exist"""
    g = torch.Generator().manual_seed(seed)
    per = n // clouds
    xyz, batch = [], []
    for b in range(clouds):
        m = per if b < clouds - 1 else n - per * (clouds - 1)
        p = torch.stack([torch.randint(0, 2 ** depth, (8 * m,), generator=g), torch.randint(0, 2 ** depth, (8 * m,), generator=g),
                         torch.randint(250, 254, (8 * m,), generator=g)], 1)
        p = torch.unique(p, dim=0)
        xyz.append(p[torch.randperm(len(p), generator=g)[:m]])
        batch.append(torch.full((m,), b))
    return torch.cat(xyz).cuda(), torch.cat(batch).cuda()


def step_of(level, C, H, D):
    R = 2 * octformer.pos_bnd_of(K, D) + 1
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(level.n, C, device="cuda", generator=g, requires_grad=True)
    w = torch.randn(27, 1, C, device="cuda", generator=g, requires_grad=True)
    qkv = torch.randn(level.n, 3 * C, device="cuda", generator=g, requires_grad=True)
    table = (0.02 * torch.randn(3 * R, H, device="cuda", generator=g)).requires_grad_(True)
    go = torch.randn(level.n, C, device="cuda", generator=g)

    def step():
        y = octformer.octree_dwconv(x, w, level)
        out = octformer.octree_attention(qkv, level, table, K, D, (C // H) ** -0.5)
        return torch.autograd.grad((y, out), (x, w, qkv, table), (go, go))

    return step


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


def launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:   # no device tracer: the count is not reported
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    for n, C, H in SIZES:
        level = octformer.octree_level(*scene(n), 9)
        for D in (1, 4):
            step = step_of(level, C, H, D)
            ms, mem, cnt = {"hip": [], "torch": []}, {}, {}
            for how in ms:   # warm-up, peak memory and launches
                os.environ["AO_AMD_OCTFORMER"] = how
                for _ in range(3):
                    step()
                mem[how], cnt[how] = peak(step), launches(step)
            for _ in range(args.rounds):   # alternating
                for how in ms:
                    os.environ["AO_AMD_OCTFORMER"] = how
                    ms[how].append(timed(step, args.iters))
            med = {how: statistics.median(v) for how, v in ms.items()}
            print(json.dumps(dict(n=n, C=C, H=H, K=K, D=D, hip_ms=round(med["hip"], 4), torch_ms=round(med["torch"], 4),
                                  speedup=round(med["torch"] / med["hip"], 2), hip_min_ms=round(min(ms["hip"]), 4),
                                  torch_min_ms=round(min(ms["torch"]), 4), hip_peak_mb=round(mem["hip"] / 2 ** 20, 2),
                                  torch_peak_mb=round(mem["torch"] / 2 ** 20, 2), hip_launches=cnt["hip"], torch_launches=cnt["torch"],
                                  rounds=args.rounds, iters=args.iters)), flush=True)


if __name__ == "__main__":
    main()
