"""Stratified Transformer: window attention on its three paths at the size of one level of a real scene, the pair lists, and
one training step of the model.

    python tools/bench_stratified.py [--points 120000] [--window 0.2] [--quant 0.01] [--heads 6] [--repeats 7] [--warmup 2]
                                     [--step-points 40000] [--no-step] [--no-eager]

Attention: a crop of --points points of a synthetic room on a 0.02 m grid (ao_amd.synth.room_scene) is sampled to a quarter by farthest point sampling -- the
points of ST-v1m2's first level -- and a quarter of those are the sampled keys of the large windows.  build_pairs (plain
windows) is timed, then forward + backward of ops.window_attention with --heads heads of 16 channels and tables of
2 * quant_grid_length rows on the paths AO_AMD_ST=fused, staged and torch, ALTERNATING between the paths in every round.
Per path: median, least and largest time per call of --repeats rounds after --warmup (a round repeats the call for about
0.2 s), the host clock around calls that end in a device synchronise, and the allocator's peak over one call above what the inputs hold.  The outputs of the three paths are compared
at that size.  The step: the reference's default ST-v1m2 (drop_path_rate 0) on a room of --step-points, forward + loss +
backward, fused and staged alternating.  One JSON line per figure, printed and written to profiles/stratified_bench.jsonl; the
last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def alternate(fn, paths, repeats, warmup, window_ms=200.0):
    """{path: figures}: the paths take turns inside every round; a round of one path repeats the call until about window_ms
    have passed (counted in the warm-up rounds), so that a call of a few milliseconds is not a measurement of the clock"""
    import torch

    wall, calls = {p: [] for p in paths}, {p: 1 for p in paths}
    for r in range(warmup + repeats):
        for p in paths:
            os.environ["AO_AMD_ST"] = p
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[p]):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / calls[p]
            if r >= warmup:
                wall[p].append(ms)
            else:
                calls[p] = max(1, min(200, int(window_ms / max(ms, 1e-3))))
    out = {}
    for p in paths:
        os.environ["AO_AMD_ST"] = p
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        out[p] = dict(ms=round(statistics.median(wall[p]), 3), min_ms=round(min(wall[p]), 3), max_ms=round(max(wall[p]), 3),
                      repeats=repeats, calls_per_repeat=calls[p], peak_mb=round(peak / 2 ** 20, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--quant", type=float, default=0.01)
    ap.add_argument("--heads", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-points", type=int, default=40000)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib, stratified, synth
    from ao_amd.pointops2 import pointops as P2

    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def scene_of(points, seed):
        """a crop of `points` points of a 10 m x 8 m room sampled on a 0.02 m grid, ScanNet's voxel size"""
        pts = synth.room_scene(seed=seed, room=1, point_max=points, density=6000.0, voxel=0.02)
        assert pts.shape[0] == points, (pts.shape, points)
        return pts

    def fps_quarter(coords):
        n = coords.shape[0]
        off = torch.tensor([n], dtype=torch.int32, device="cuda")
        new = torch.tensor([n // 4 + 1], dtype=torch.int32, device="cuda")
        return P2.furthestsampling(coords, off, new).long()

    room = torch.from_numpy(scene_of(args.points, 0)).float().cuda()
    coords = room[fps_quarter(room)].contiguous()
    n, h, hd = coords.shape[0], args.heads, 16
    offset = torch.tensor([n], dtype=torch.int32, device="cuda")
    down_idx = fps_quarter(coords)
    rows_l = 2 * stratified.quant_grid_length(args.window, args.quant)
    os.environ["AO_AMD_ST"] = "fused"
    timing = alternate(lambda: stratified.build_pairs(coords, offset, down_idx, args.window, False), ["fused"], args.repeats, args.warmup)
    pairs = stratified.build_pairs(coords, offset, down_idx, args.window, False)
    emit(figure="build_pairs", points=n, sampled=int(down_idx.numel()), window=args.window, pairs=pairs.m, n_max=pairs.n_max,
         mean_row=round(pairs.m / n, 1), one_Mh_array_mb=round(pairs.m * h * 4 / 2 ** 20, 1), **timing["fused"])

    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(n, h, hd, device="cuda", generator=g).requires_grad_(True) for _ in range(3))
    with torch.no_grad():
        q.mul_(hd ** -0.5)
    tables = [(0.02 * torch.randn(rows_l, h, hd, 3, device="cuda", generator=g)).requires_grad_(True) for _ in range(3)]
    g_out = torch.randn(n, h * hd, device="cuda", generator=g)
    leaves = [q, k, v] + tables

    def attention():
        out = stratified.window_attention(q, k, v, coords, pairs, *tables, args.window, args.quant)
        return (out,) + torch.autograd.grad(out, leaves, g_out)

    paths = ["fused", "staged"] + ([] if args.no_eager else ["torch"])
    timing = alternate(attention, paths, args.repeats, args.warmup)
    results = {}
    for p in paths:
        os.environ["AO_AMD_ST"] = p
        results[p] = [t.detach().clone() for t in attention()]
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    agree = {p: round(max(rel(a, b) for a, b in zip(results[p], results["fused"])), 9) for p in paths if p != "fused"}
    row = dict(figure="window_attention_fwd_bwd", points=n, heads=h, channels_per_head=hd, table_rows=rows_l, pairs=pairs.m,
               largest_relative_l2_to_fused=agree, **timing)
    for p in paths[1:]:
        row[p + "_over_fused"] = round(timing[p]["ms"] / timing["fused"]["ms"], 2)
    emit(**row)
    del results

    if not args.no_step:
        torch.manual_seed(0)
        model = stratified.StratifiedTransformer(in_channels=6, num_classes=20, drop_path_rate=0.0).cuda().train()
        scene = torch.from_numpy(scene_of(args.step_points, 1)).float().cuda()
        rng = np.random.default_rng(0)
        batch = dict(coord=scene, feat=torch.cat([scene, torch.from_numpy(rng.uniform(0, 1, (args.step_points, 3)).astype(np.float32)).cuda()], 1),
                     offset=torch.tensor([args.step_points], dtype=torch.int32, device="cuda"))
        segment = torch.from_numpy(rng.integers(0, 20, scene.shape[0])).cuda()

        def step():
            model.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(batch), segment).backward()

        emit(figure="train_step", config="ST-v1m2 defaults, drop_path_rate 0", points=args.step_points,
             **alternate(step, ["fused", "staged"], max(3, args.repeats // 2), 1))
    emit(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0), numpy=np.__version__,
         torch=torch.__version__)
    with open(os.path.join(ROOT, "profiles", "stratified_bench.jsonl"), "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
