"""CAC-v1m1 heads: native (ao_amd/csrc/cac.hip) against the eager formulation (AO_AMD_CAC=torch), and a whole ScanNet-config
step of the CAC segmentor against DefaultSegmentor with the same criteria.

    python tools/bench_cac.py            # every section, each in a child process under `timeout -k 10`
    python tools/bench_cac.py heads      # one section in this process

Prints one JSON line per measurement.  heads: the CAC-specific work of a training step at 3 x 100 k rows, C = 48 -- soft
prototypes, proj, feat_proj_layer (per scene and whole batch), class means, apd_proj, both cosine logits and the distillation
loss, forward + backward, WITHOUT the three criteria evaluations -- median ms over --iters, launches per call (kernels and
memsets seen by the profiler), host synchronisations per call (torch's sync debug mode).  step: forward + backward + FlatAdamW
of the ScanNet CAC config (CE + Lovasz, 20 classes) at 2 x 100 k points, CAC native / CAC eager heads / DefaultSegmentor."""
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

SIZES = [(20, 0.75), (200, 0.0)]  # classes, conf_thresh (the ScanNet and ScanNet200 CAC configs)
ROWS = [100000, 100000, 100000]
SECTIONS = {"heads": 600, "step": 900}


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


def section_heads(iters):
    import torch

    from ao_amd.ptv2 import CACSegmentor
    from ao_amd.ptv2.cac import distill_loss

    class Identity(torch.nn.Module):
        def forward(self, d):
            return d["feat"]

    n = sum(ROWS)
    bounds = [sum(ROWS[:i + 1]) for i in range(len(ROWS))]
    for k, thr in SIZES:
        torch.manual_seed(0)
        seg = CACSegmentor(k, 48, backbone=Identity(), criteria=[], conf_thresh=thr, detach_pre_logits=True).cuda().train()
        g = torch.Generator(device="cuda").manual_seed(1)
        feat = (torch.randn(n, 48, generator=g, device="cuda") * 2).requires_grad_(True)
        label = torch.randint(0, k, (n,), generator=g, device="cuda")
        label[torch.rand(n, generator=g, device="cuda") < 0.1] = -1
        offset = torch.tensor(bounds, dtype=torch.int32, device="cuda")
        logits = seg.seg_head(feat).detach()

        def fn():
            feat.grad = None
            refine = seg.refine_logits(feat, logits, bounds, offset)
            cac = seg.adaptive_logits(feat, label, bounds, offset)
            (distill_loss(refine, cac.detach(), label) + refine.mean() + cac.mean()).backward()

        row = dict(rows=n, classes=k, conf_thresh=thr, channels=48)
        for mode in ("hip", "torch"):
            os.environ["AO_AMD_CAC"] = mode
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            row[mode] = dict(ms=round(_time(fn, iters), 4), launches=_launches(fn), syncs=_syncs(fn))
        row["speedup"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row), flush=True)
    os.environ.pop("AO_AMD_CAC", None)


def section_step(iters):
    import torch

    import ao_amd.ptv2 as ptv2
    from ao_amd import synth
    from ao_amd.ptv2.optim import FlatAdamW

    cfg = dict(ptv2.SCANNET_BACKBONE)
    b = synth.scene_batch([0, 1], point_max=100000, in_channels=9, num_classes=20, room=2)
    data = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    data["offset_host"] = b["offset"].tolist()
    ce = dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)
    lov = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)
    out = dict(points=int(data["coord"].shape[0]))
    for tag, mode in (("default", "hip"), ("cac", "hip"), ("cac_eager_heads", "torch")):
        os.environ["AO_AMD_CAC"] = mode
        torch.manual_seed(0)
        if tag == "default":
            seg = ptv2.DefaultSegmentor(cfg, criteria=[ce, lov]).cuda().train()
        else:
            seg = ptv2.CACSegmentor(20, 48, backbone=dict(cfg, num_classes=0), criteria=[ce, lov], conf_thresh=0.75,
                                    detach_pre_logits=True).cuda().train()
        opt = FlatAdamW(seg.parameters(), lr=0.005, weight_decay=0.02)

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
    out["cac_added_ms"] = round(out["cac_ms"] - out["default_ms"], 3)
    out["cac_eager_heads_added_ms"] = round(out["cac_eager_heads_ms"] - out["default_ms"], 3)
    print(json.dumps(out), flush=True)
    os.environ.pop("AO_AMD_CAC", None)


def main():
    args = sys.argv[1:]
    iters = 20
    if "--iters" in args:
        i = args.index("--iters")
        iters = int(args[i + 1])
        del args[i:i + 2]
    if args:
        {"heads": section_heads, "step": section_step}[args[0]](iters)
        return
    for name, limit in SECTIONS.items():  # each section in a child of its own: a fault ends the run there
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name,
                              "--iters", str(iters)])
        if rc != 0:
            print(json.dumps(dict(section=name, exit=rc)), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
