#!/usr/bin/env python
"""Times one Swin3D block's attention (crse_attention), forward + backward, on ao_amd/csrc/swin_attention.hip against the eager
statements (AO_AMD_SWIN3D=torch) on the same device: warm-up, alternating rounds, medians, peak memory above the inputs (DESIGN.md
section 21).  Shapes: level 0 and level 2 of the small config, full cRSE.

    python tools/bench_swin3d.py [--rounds 15] [--iters 10]

One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import swin3d  # noqa: E402

SIZES = [(40000, 48, 6, 5), (5000, 192, 12, 7)]   # n, C, H, window_size
QUANT = 4


def scene(n, clouds=2, seed=0):
    """n unique voxels on a slab four voxels thick at a quarter of full density, so that windows hold tens of members"""
    g = torch.Generator().manual_seed(seed)
    per = n // clouds
    edge = int(per ** 0.5) + 1
    xyz, batch = [], []
    for b in range(clouds):
        p = torch.cat([torch.randint(0, edge, (8 * per, 2), generator=g), torch.randint(250, 254, (8 * per, 1), generator=g)], 1)
        p = torch.unique(p, dim=0)
        xyz.append(p[torch.randperm(len(p), generator=g)[:per]])
        batch.append(torch.full((per,), b))
    return torch.cat(xyz).cuda(), torch.cat(batch).cuda()


def step_of(wmap, C, H, ws):
    n, rows = wmap.n, (ws * QUANT, 4 * QUANT, 4 * QUANT)
    g = torch.Generator(device="cuda").manual_seed(1)
    local = torch.rand(n, 3, device="cuda", generator=g)
    colors = torch.rand(n, 6, device="cuda", generator=g) * 2 - 1
    signals = swin3d.crse_signals(wmap, local, colors, QUANT, "XYZ_RGB_NORM")
    qkv = torch.randn(n, 3 * C, device="cuda", generator=g, requires_grad=True)
    tables = [(0.02 * torch.randn(6 * sum(rows) * C, device="cuda", generator=g)).requires_grad_(True) for _ in range(3)]
    go = torch.randn(n, C, device="cuda", generator=g)

    def step():
        out = swin3d.crse_attention(qkv, wmap, signals, *tables, rows, (C // H) ** -0.5, H)
        return torch.autograd.grad(out, [qkv] + tables, go)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    for n, C, H, ws in SIZES:
        wmap = swin3d.window_map(*scene(n), ws, 0)
        pairs = int(((wmap.offsets[1:] - wmap.offsets[:-1]).long() ** 2).sum())
        step = step_of(wmap, C, H, ws)
        ms, mem = {"hip": [], "torch": []}, {}
        for how in ms:   # warm-up and peak memory
            os.environ["AO_AMD_SWIN3D"] = how
            for _ in range(3):
                step()
            mem[how] = peak(step)
        for _ in range(args.rounds):   # alternating
            for how in ms:
                os.environ["AO_AMD_SWIN3D"] = how
                ms[how].append(timed(step, args.iters))
        med = {how: statistics.median(v) for how, v in ms.items()}
        print(json.dumps(dict(n=wmap.n, C=C, H=H, window_size=ws, windows=wmap.W, m_max=wmap.m_max, pairs=pairs,
                              hip_ms=round(med["hip"], 4), torch_ms=round(med["torch"], 4), speedup=round(med["torch"] / med["hip"], 2),
                              hip_min_ms=round(min(ms["hip"]), 4), torch_min_ms=round(min(ms["torch"]), 4),
                              hip_peak_mb=round(mem["hip"] / 2 ** 20, 2), torch_peak_mb=round(mem["torch"] / 2 ** 20, 2),
                              rounds=args.rounds, iters=args.iters)), flush=True)


if __name__ == "__main__":
    main()
