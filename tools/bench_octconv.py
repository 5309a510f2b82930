#!/usr/bin/env python
"""Times OctFormer's dense octree convolutions, forward + backward, on ao_amd/csrc/oct_conv.hip (--operands fp32), on
ao_amd/csrc/oct_conv_bf16.hip (bf16) or on both, against the eager fp32 slot loop (AO_AMD_OCTFORMER=torch) on the same device: warm-up, alternating runs, medians, peak memory above the inputs and the device
launches of one forward + backward (DESIGN.md sections 23 and 24).  The eager loop is a description of cost, not a tuned baseline.

    python tools/bench_octconv.py [--rounds 15] [--iters 10] [--nodes 40000] [--operands fp32|bf16|both]

One JSON line per (form, Cin, Cout)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import octformer  # noqa: E402
from tools.bench_octformer import launches, peak, scene, timed  # noqa: E402

PAIRS = [(168, 168), (24, 48)]
HOW = {"hip": ("hip", "fp32"), "bf16": ("hip", "bf16"), "torch": ("torch", "fp32")}   # AO_AMD_OCTFORMER, operands


OPERANDS = ["fp32"]   # of the variant being run


def select(how):
    os.environ["AO_AMD_OCTFORMER"], OPERANDS[0] = HOW[how]


def step_of(pyramid, form, cin, cout):
    link = pyramid.link(pyramid.depth)
    table = pyramid.level(pyramid.depth) if form == "conv3" else link
    n_in = link.n_parent if form == "deconv3" else link.n
    slots = 8 if form == "down2" else 27
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n_in, cin, device="cuda", generator=g, requires_grad=True)
    w = torch.randn((slots, cout, cin) if form == "deconv3" else (slots, cin, cout), device="cuda", generator=g, requires_grad=True)
    b = torch.randn(cout, device="cuda", generator=g, requires_grad=True) if form == "down2" else None
    go = torch.randn(link.n_parent if form == "down2" else link.n, cout, device="cuda", generator=g)

    def step():
        y = octformer.octree_conv(x, w, b, table, form, operands=OPERANDS[0])
        return torch.autograd.grad(y, (x, w) if b is None else (x, w, b), go)

    return step, n_in, go.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=40000)
    ap.add_argument("--operands", choices=("fp32", "bf16", "both"), default="fp32")
    args = ap.parse_args()
    hows = {"fp32": ["hip"], "bf16": ["bf16"], "both": ["hip", "bf16"]}[args.operands] + ["torch"]
    pyramid = octformer.octree_pyramid(*scene(args.nodes), 9, 2)
    for form in octformer.ops.FORMS:
        for cin, cout in PAIRS:
            step, n_in, n_out = step_of(pyramid, form, cin, cout)
            ms, mem, cnt = {how: [] for how in hows}, {}, {}
            for how in ms:   # warm-up, peak memory and launches
                select(how)
                for _ in range(3):
                    step()
                mem[how], cnt[how] = peak(step), launches(step)
            for _ in range(args.rounds):   # alternating
                for how in ms:
                    select(how)
                    ms[how].append(timed(step, args.iters))
            med = {how: statistics.median(v) for how, v in ms.items()}
            row = dict(form=form, cin=cin, cout=cout, n_in=n_in, n_out=n_out)
            for how in hows:
                row.update({how + "_ms": round(med[how], 4), how + "_min_ms": round(min(ms[how]), 4),
                            how + "_peak_mb": round(mem[how] / 2 ** 20, 2), how + "_launches": cnt[how]})
                if how != "torch":
                    row["speedup" if how == "hip" else "bf16_speedup"] = round(med["torch"] / med[how], 2)
            print(json.dumps(dict(row, rounds=args.rounds, iters=args.iters)), flush=True)


if __name__ == "__main__":
    main()
