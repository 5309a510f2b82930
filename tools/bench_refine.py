"""REAL's epoch-end label refinement of one synthetic room: device time per stage against the numpy restatement.

    python tools/bench_refine.py [--points 1000000] [--classes 13] [--views 4] [--repeats 5] [--warmup 1] [--inner 20]

The room is tests/refine_cases.make_room (unsettled: a timing run compares no choices), the masks are discs around the
prompts, made once and served to both sides.  Stages: confidence (pred + softmax margin), prompts (the grid search, with its
one count read), vote (all views, masks given), update.  The host side is tests/refine_ref.py, which is VECTORISED numpy: the
reference's own triple python loop over cells x classes (train_sam_real.py:362-388, a full-n mask per iteration) is slower
than that and is not timed here.  One JSON line per stage; the last line carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup, device=True, inner=1):
    """median / min / max over `repeats` samples of the host clock around `inner` calls that end in a device synchronise"""
    import torch

    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        if device:
            torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / inner)
    return dict(ms=round(statistics.median(wall), 3), min=round(min(wall), 3), max=round(max(wall), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=20, help="device calls per timed sample (the short stages are tens of microseconds)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib
    from ao_amd.ptv2 import refine as R
    from tests import refine_cases as RC
    from tests import refine_ref as RR

    n, c, size = args.points, args.classes, 128
    case = RC.make_room("bench", 1, n, c, 12.0, 9.0, absent=(5,), views=args.views, height=size, width=size, settled=False)
    label = case["label"].reshape(-1)
    pred, conf = RR.confidence(case["logits"])
    prompt_idx, prompt_cls = RR.prompts(case["coord"], pred, conf, label, case["present"])
    seen = [np.nonzero(b[prompt_idx, 2] == 1)[0] for b in case["bridges"]]
    masks = [RC.masks_for(case, v, b[prompt_idx[s], :2], prompt_cls[s]) for v, (b, s) in enumerate(zip(case["bridges"], seen))]

    dev = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)  # noqa: E731
    logits_d, coord_d, label_d, present_d = dev(case["logits"]), dev(case["coord"]), dev(label, torch.int32), dev(case["present"])
    bridges_d, masks_d = [dev(b, torch.int32) for b in case["bridges"]], [dev(m) for m in masks]
    lo, hi = case["coord"].min(0), case["coord"].max(0)
    bounds = (lo[0], hi[0], lo[1], hi[1])
    refiner = R.LabelRefiner(c).begin(logits_d, coord_d, label_d, present_d, bounds)
    pred_d, conf_d = refiner.pred, refiner.conf

    def vote_device():
        refiner.vote.zero_()
        for v, bridge in enumerate(bridges_d):
            refiner.vote_view(bridge, lambda xy, k, _v=v: masks_d[_v])

    def update_device():
        refiner.label.copy_(label_d)
        refiner.touched = True
        refiner.finish(check=False)

    vote_host = np.zeros((n, c), np.int32)

    def vote_numpy():
        vote_host[:] = 0
        for v, bridge in enumerate(case["bridges"]):
            RR.vote_view(vote_host, bridge, pred, conf, prompt_idx, prompt_cls, lambda uv, k, _v=v: masks[_v])

    stages = [
        ("confidence", lambda: R.scene_confidence(logits_d), lambda: RR.confidence(case["logits"])),
        ("prompts", lambda: R.grid_prompts(coord_d, pred_d, conf_d, label_d, present_d, bounds=bounds),
         lambda: RR.prompts(case["coord"], pred, conf, label, case["present"])),
        ("vote", vote_device, vote_numpy),
        ("update", update_device, lambda: RR.update(vote_host, pred, label)),
    ]
    total_d = total_h = 0.0
    for name, on_device, on_host in stages:
        d = timed(on_device, args.repeats, args.warmup, inner=args.inner)
        h = timed(on_host, max(1, args.repeats // 2), min(args.warmup, 1), device=False)
        total_d, total_h = total_d + d["ms"], total_h + h["ms"]
        print(json.dumps(dict(stage=name, device=d, numpy=h)))
    same = bool(np.array_equal(refiner.vote.cpu().numpy(), vote_host))
    print(json.dumps(dict(points=n, classes=c, views=args.views, image=[size, size], prompts=int(prompt_idx.size),
                          prompts_seen=[int(s.size) for s in seen], device_ms=round(total_d, 3), numpy_ms=round(total_h, 3),
                          votes_equal=same, build=_lib.lib().ptv2_build_info().decode())))


if __name__ == "__main__":
    main()
