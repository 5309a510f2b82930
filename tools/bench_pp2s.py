"""The PP2S label pipeline of one synthetic room: device time per stage against the numpy restatement.

    python tools/bench_pp2s.py [--points 1000000] [--classes 13] [--views 24] [--image 1080] [--repeats 5] [--warmup 1]

The room is a box of uniform points with an instance per 0.75 m patch of the floor plan (about 200), the views are the
pinhole cameras of tests/pp2s_cases.make_views on square images whose depth is rendered from the points, the masks are discs
around the prompts, made once and served to both sides: the mask predictor is outside every figure, and so are the uploads of
the depth images and the masks.  Stages: align, project (all views), weak, prompts (view_prompts of all views, one read each),
vote (all views), labels; the vote's two passes are also timed on their own (the masks' stream, the per-point gather).  The
host side is tests/pp2s_ref.py, which is VECTORISED numpy: the reference's own python loops (my_run_sam_final.py:100, one
iteration per visible point and prompt) are slower than that and are not timed here.  The host clock around calls that end in
a device synchronise; repeats re-read inputs that the caches may still hold.  One JSON line per stage; the last line says
whether the two sides' bridges and labels are equal and carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup, device=True):
    """median / min / max over `repeats` samples of the host clock around one call that ends in a device synchronise"""
    import torch

    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device:
            torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(wall), 3), min=round(min(wall), 3), max=round(max(wall), 3))


def discs(rng, xy, size):
    """(P, size, size) bool: a disc of 40..160 pixels radius around every prompt's element [y - 1][x - 1]"""
    import numpy as np

    out = np.zeros((len(xy), size, size), bool)
    for p, (x, y) in enumerate(xy):
        radius = int(rng.integers(40, 160))
        r0, r1, c0, c1 = max(y - 1 - radius, 0), min(y + radius, size), max(x - 1 - radius, 0), min(x + radius, size)
        rr, cc = np.mgrid[r0:r1, c0:c1]
        out[p, r0:r1, c0:c1] = (rr - (y - 1)) ** 2 + (cc - (x - 1)) ** 2 <= radius ** 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--image", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib
    from ao_amd.ptv2 import pp2s as P
    from tests import pp2s_cases as PC
    from tests import pp2s_ref as PR

    n, c, size = args.points, args.classes, args.image
    rng = np.random.default_rng(1)
    box_x, box_y, angle, center = 12.0, 9.0, 33, np.array([3.6125, 2.2875, 1.4375])
    local = (rng.random((n, 3)) - 0.5) * np.array([box_x, box_y, 2.8])
    rot_cos, rot_sin = PR.rotation(angle)
    raw = np.stack([local[:, 0] * rot_cos + local[:, 1] * rot_sin, -local[:, 0] * rot_sin + local[:, 1] * rot_cos, local[:, 2]], 1)
    coord = (raw + center).astype(np.float32)
    patch = np.floor((local[:, 0] + box_x / 2) / 0.75).astype(np.int64) * 12 + np.floor((local[:, 1] + box_y / 2) / 0.75).astype(np.int64)
    instance = (patch * 37 + 5).astype(np.int32)
    semantic = ((patch * 7 + 3) % c).astype(np.int32)
    coord64 = PR.align(coord, angle, center)
    views = PC.make_views(rng, coord64, center, box_x, box_y, args.views + 1, (size, size))[:args.views]  # (the last looks away)
    depths = [v["depth"] / PC.DEPTH_SCALE for v in views]

    # the host side once, for the inputs of the later stages
    bridges = [PR.project(coord64, v["k"], v["rt"], d, PC.TOL)[0] for v, d in zip(views, depths)]
    seen_any = np.zeros(n, np.uint8)
    for b in bridges:
        seen_any[b[:, 2] == 1] = 1
    weak = PR.weak_mask(instance, seen_any)
    prompts = [PR.view_prompts(b, weak, semantic) for b in bridges]
    masks = [discs(rng, xy, size) for _, xy, _ in prompts]

    dev = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)  # noqa: E731
    coord_d, instance_d, semantic_d = dev(coord), dev(instance), dev(semantic)
    depths_d, masks_d, cls_d = [dev(d) for d in depths], [dev(m) for m in masks], [dev(k) for _, _, k in prompts]
    coord64_d = P.align_room(coord_d, angle, center)
    state = {}

    def project_device():
        state["seen_any"] = torch.zeros(n, dtype=torch.uint8, device="cuda")
        state["bridges"] = [P.project_view(coord64_d, v["k"], v["rt"], d, depth_scale=1, seen_any=state["seen_any"])[0]
                            for v, d in zip(views, depths_d)]

    project_device()
    weak_d = P.choose_weak_labels(instance_d, state["seen_any"])
    prop = P.LabelPropagator(semantic_d, weak_d, c)

    def vote_device():
        prop.seen_bits.zero_()
        for b, m, k in zip(state["bridges"], masks_d, cls_d):
            prop.vote_view(b, m, k)

    seen_bits = np.zeros(n, np.uint32)

    def vote_numpy():
        seen_bits[:] = 0
        for b, m, (_, _, k) in zip(bridges, masks, prompts):
            PR.vote_view(seen_bits, b, m, k, c)

    # the vote's two passes on their own
    L = _lib.lib()
    ws = _lib.workspace(L.pp2s_workspace_bytes(0, size, size), coord_d.device)

    def pass_a():
        for m, k in zip(masks_d, cls_d):
            L.pp2s_pixel_labels_hip_launcher(k.shape[0], c, k.data_ptr(), m.data_ptr(), size, size, ws.data_ptr(), ws.numel(),
                                             prop.status.data_ptr(), _lib.stream_ptr())

    def pass_b():
        for b in state["bridges"]:
            L.pp2s_vote_hip_launcher(n, b.data_ptr(), size, size, ws.data_ptr(), ws.numel(), prop.seen_bits.data_ptr(),
                                     prop.status.data_ptr(), _lib.stream_ptr())

    stages = [
        ("align", lambda: P.align_room(coord_d, angle, center), lambda: PR.align(coord, angle, center)),
        ("project", project_device, lambda: [PR.project(coord64, v["k"], v["rt"], d, PC.TOL) for v, d in zip(views, depths)]),
        ("weak", lambda: P.choose_weak_labels(instance_d, state["seen_any"]), lambda: PR.weak_mask(instance, seen_any)),
        ("prompts", lambda: [prop.view_prompts(b) for b in state["bridges"]],
         lambda: [PR.view_prompts(b, weak, semantic) for b in bridges]),
        ("vote", vote_device, vote_numpy),
        ("vote.pixel_labels", pass_a, None),
        ("vote.gather", pass_b, None),
        ("labels", lambda: prop.finish(check=False), lambda: PR.labels(seen_bits, weak, semantic)),
    ]
    total_d = total_h = 0.0
    for name, on_device, on_host in stages:
        d = timed(on_device, args.repeats, args.warmup)
        line = dict(stage=name, device=d)
        if on_host is not None:
            h = timed(on_host, max(1, args.repeats // 2), min(args.warmup, 1), device=False)
            total_d, total_h = total_d + d["ms"], total_h + h["ms"]
            line["numpy"] = h
        print(json.dumps(line), flush=True)
    vote_device()
    label = prop.finish().cpu().numpy()
    same_bridges = all(np.array_equal(b.cpu().numpy(), ref) for b, ref in zip(state["bridges"], bridges))
    same_labels = bool(np.array_equal(label, PR.labels(seen_bits, weak, semantic)))
    mask_bytes = sum(int(m.size) for m in masks)
    print(json.dumps(dict(points=n, classes=c, views=args.views, image=[size, size], instances=int(np.unique(instance).size),
                          visible=[int(b[:, 2].sum()) for b in bridges], prompts_seen=[int(p[0].size) for p in prompts],
                          mask_bytes=mask_bytes, labelled=int((label != -1).sum()), device_ms=round(total_d, 3),
                          numpy_ms=round(total_h, 3), bridges_equal=same_bridges, labels_equal=same_labels,
                          build=_lib.lib().ptv2_build_info().decode())))


if __name__ == "__main__":
    main()
