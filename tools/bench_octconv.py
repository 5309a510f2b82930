#!/usr/bin/env python
"""Times OctFormer's dense octree convolutions, forward + backward, on ao_amd/csrc/oct_conv.hip against the eager slot loop
(AO_AMD_OCTFORMER=torch) on the same device: warm-up, alternating runs, medians, peak memory above the inputs and the device
launches of one forward + backward.  The eager loop is a description of cost, not a tuned baseline.

    python tools/bench_octconv.py [--rounds 15] [--iters 10] [--nodes 40000]

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
        y = octformer.octree_conv(x, w, b, table, form)
        return torch.autograd.grad(y, (x, w) if b is None else (x, w, b), go)

    return step, n_in, go.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=40000)
    args = ap.parse_args()
    pyramid = octformer.octree_pyramid(*scene(args.nodes), 9, 2)
    for form in octformer.ops.FORMS:
        for cin, cout in PAIRS:
            step, n_in, n_out = step_of(pyramid, form, cin, cout)
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
            print(json.dumps(dict(form=form, cin=cin, cout=cout, n_in=n_in, n_out=n_out, hip_ms=round(med["hip"], 4),
                                  torch_ms=round(med["torch"], 4), speedup=round(med["torch"] / med["hip"], 2),
                                  hip_min_ms=round(min(ms["hip"]), 4), torch_min_ms=round(min(ms["torch"]), 4),
                                  hip_peak_mb=round(mem["hip"] / 2 ** 20, 2), torch_peak_mb=round(mem["torch"] / 2 ** 20, 2),
                                  hip_launches=cnt["hip"], torch_launches=cnt["torch"], rounds=args.rounds, iters=args.iters)), flush=True)


if __name__ == "__main__":
    main()
