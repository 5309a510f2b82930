#!/usr/bin/env python
"""Times one Swin3D block's attention (crse_attention), forward + backward, on ao_amd/csrc/swin_attention.hip against the eager
statements (AO_AMD_SWIN3D=torch) on the same device: warm-up, alternating rounds, medians, peak memory above the inputs (DESIGN.md
section 21).  Shapes: level 0 and level 2 of the small config, full cRSE.

    python tools/bench_swin3d.py [--rounds 15] [--iters 10] [--half]

--half times the half-precision path instead (ao_amd/csrc/swin_attention_f16.hip): the same float16 qkv
under fp16 autocast with fp16_mode=1 ("f16") and with fp16_mode=0 ("fp32": what an autocast user got before the path existed,
the cast of qkv to fp32 included), and reports the forward's resident workgroups per compute unit.

One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import _lib, swin3d  # noqa: E402

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


def step_of(wmap, C, H, ws, fp16_mode=None):
    """forward + backward of crse_attention on an fp32 qkv, or with fp16_mode on a float16 qkv under fp16 autocast"""
    n, rows = wmap.n, (ws * QUANT, 4 * QUANT, 4 * QUANT)
    g = torch.Generator(device="cuda").manual_seed(1)
    local = torch.rand(n, 3, device="cuda", generator=g)
    colors = torch.rand(n, 6, device="cuda", generator=g) * 2 - 1
    signals = swin3d.crse_signals(wmap, local, colors, QUANT, "XYZ_RGB_NORM")
    qkv = torch.randn(n, 3 * C, device="cuda", generator=g)
    qkv = (qkv if fp16_mode is None else qkv.half()).requires_grad_(True)
    tables = [(0.02 * torch.randn(6 * sum(rows) * C, device="cuda", generator=g)).requires_grad_(True) for _ in range(3)]
    go = torch.randn(n, C, device="cuda", generator=g)

    def step():
        with torch.autocast("cuda", dtype=torch.float16, enabled=fp16_mode is not None):
            out = swin3d.crse_attention(qkv, wmap, signals, *tables, rows, (C // H) ** -0.5, H, fp16_mode=fp16_mode or 0)
        return torch.autograd.grad(out, [qkv] + tables, go.to(out.dtype))

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


def alternate(steps, rounds, iters):
    """{name: (median ms, min ms, peak bytes)}: warm-up and peak memory, then alternating rounds"""
    ms, mem = {k: [] for k in steps}, {}
    for k, step in steps.items():
        for _ in range(3):
            step()
        mem[k] = peak(step)
    for _ in range(rounds):
        for k, step in steps.items():
            ms[k].append(timed(step, iters))
    return {k: (statistics.median(v), min(v), mem[k]) for k, v in ms.items()}


def main_half(args):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n, C, H, ws in SIZES:
        wmap = swin3d.window_map(*scene(n), ws, 0)
        res = alternate({"f16": step_of(wmap, C, H, ws, 1), "fp32": step_of(wmap, C, H, ws, 0)}, args.rounds, args.iters)
        resident = _lib.lib().ptv2_swin_f16_fwd_resident_blocks(C // H, 3, 6 * (ws * QUANT + 8 * QUANT))
        print(json.dumps(dict(n=wmap.n, C=C, H=H, window_size=ws, windows=wmap.W, m_max=wmap.m_max,
                              f16_ms=round(res["f16"][0], 4), fp32_ms=round(res["fp32"][0], 4),
                              speedup=round(res["fp32"][0] / res["f16"][0], 2), f16_min_ms=round(res["f16"][1], 4),
                              fp32_min_ms=round(res["fp32"][1], 4), f16_peak_mb=round(res["f16"][2] / 2 ** 20, 2),
                              fp32_peak_mb=round(res["fp32"][2] / 2 ** 20, 2), f16_fwd_resident_workgroups=resident,
                              compute_units=cus, f16_fwd_workgroups_per_cu=round(resident / cus, 2), rounds=args.rounds,
                              iters=args.iters)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--half", action="store_true", help="time fp16_mode=1 beside fp16_mode=0 on a float16 qkv under autocast")
    args = ap.parse_args()
    if args.half:
        return main_half(args)
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
