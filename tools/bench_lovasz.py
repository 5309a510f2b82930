"""Lovasz-softmax loss: native (ao_amd/csrc/lovasz.hip) against the eager formulation (AO_AMD_LOVASZ=torch), and what
CE + Lovasz adds to a ScanNet-config training step over CE alone.

    python tools/bench_lovasz.py            # every section, each in a child process under `timeout -k 10`
    python tools/bench_lovasz.py loss       # one section in this process

Prints one JSON line per measurement: forward + backward ms (median over --iters), launches per call (kernels and memsets
seen by the profiler) and host synchronisations per call (torch's sync debug mode); then the step times."""
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(120000, 13, 13, 1), (100000, 20, 20, 2), (200000, 200, 60, 1)]  # rows per cloud, C, classes present, clouds
SECTIONS = {"loss": 600, "step": 900}


def _inputs(n, c, present, seed=0):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    classes = torch.randperm(c, generator=g, device="cuda")[:present]
    label = classes[torch.randint(0, present, (n,), generator=g, device="cuda")]
    label[torch.rand(n, generator=g, device="cuda") < 0.1] = -1
    logits = torch.randn(n, c, generator=g, device="cuda") * 3.0
    return logits, label


def _fwd_bwd(x, label):
    from ao_amd.ptv2 import lovasz_softmax

    x.grad = None
    lovasz_softmax(x, label, -1).backward()


def _time(fn, iters):
    import torch

    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def _launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kinds = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(kinds)


def _syncs(fn):
    import torch

    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message) for x in w)


def section_loss(iters):
    import torch

    for n, c, present, clouds in SIZES:
        logits, label = _inputs(n * clouds, c, present)
        x = logits.clone().requires_grad_(True)
        row = dict(rows=n * clouds, classes=c, present=present)
        for mode in ("hip", "torch"):
            os.environ["AO_AMD_LOVASZ"] = mode
            fn = lambda: _fwd_bwd(x, label)  # noqa: E731
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            row[mode] = dict(ms=round(_time(fn, iters), 4), launches=_launches(fn), syncs=_syncs(fn))
        row["speedup"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row), flush=True)
    os.environ.pop("AO_AMD_LOVASZ", None)


def section_step(iters):
    import torch

    import ao_amd.ptv2 as ptv2
    from ao_amd import synth
    from ao_amd.ptv2.optim import FlatAdamW

    cfg = dict(ptv2.SCANNET_BACKBONE)
    b = synth.scene_batch([0, 1], point_max=100000, in_channels=9, num_classes=20, room=2)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    ce = dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)
    lov = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)
    out = dict(points=int(data["coord"].shape[0]))
    for tag, criteria, mode in (("ce", [ce], "hip"), ("ce_lovasz", [ce, lov], "hip"), ("ce_lovasz_eager", [ce, lov], "torch")):
        os.environ["AO_AMD_LOVASZ"] = mode
        torch.manual_seed(0)
        seg = ptv2.DefaultSegmentor(cfg, criteria=criteria).cuda().train()
        opt = FlatAdamW(seg.parameters(), lr=0.006, weight_decay=0.05)

        def step():
            loss = seg(data)["loss"]
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        for _ in range(3):
            step()
        ts = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        out[tag + "_ms"] = round(statistics.median(ts), 3)
        del seg, opt
        torch.cuda.empty_cache()
    out["lovasz_added_ms"] = round(out["ce_lovasz_ms"] - out["ce_ms"], 3)
    out["eager_lovasz_added_ms"] = round(out["ce_lovasz_eager_ms"] - out["ce_ms"], 3)
    print(json.dumps(out), flush=True)
    os.environ.pop("AO_AMD_LOVASZ", None)


def main():
    args = sys.argv[1:]
    iters = 20
    if "--iters" in args:
        i = args.index("--iters")
        iters = int(args[i + 1])
        del args[i:i + 2]
    if args:
        {"loss": section_loss, "step": section_step}[args[0]](iters)
        return
    for name, limit in SECTIONS.items():  # each section in a child of its own: a fault ends the run there
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name,
                              "--iters", str(iters)])
        if rc != 0:
            print(json.dumps(dict(section=name, exit=rc)), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
