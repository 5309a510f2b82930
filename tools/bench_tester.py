"""Whole-scene test-time inference of one synthetic 120 000-point room under the full S3DIS test_cfg (10 augmentations).

    python tools/bench_tester.py [--points 120000] [--repeats 5] [--warmup 1]

Legs, each timed as scene wall time and GPU time (events around the scene), median and min-max over --repeats after --warmup:
  (a) the literal loop of pointcept/engines/test.py:94-123 on this project's model (what a user can run without the tester)
  (b) ao_amd.ptv2.test_scene with fragment_batch 1, 2, 4, 8
  (c) the vote step alone over the scene's recorded logits, per fragment: eager (AO_AMD_VOTE=torch) against HIP
and the graph cache's counters over one scene of (b) (ao_amd/csrc/graph.hip; run with AO_AMD_GRAPH_DEBUG=1 to see every
capture / update as it happens).  One JSON line per measurement; the last line carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup):
    import torch

    for _ in range(warmup):
        fn()
    wall, gpu = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(a.elapsed_time(b))
    return dict(wall_ms=round(statistics.median(wall), 3), wall_min=round(min(wall), 3), wall_max=round(max(wall), 3),
                gpu_ms=round(statistics.median(gpu), 3), gpu_min=round(min(gpu), 3), gpu_max=round(max(gpu), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch

    import ao_amd.ptv2 as ptv2
    from ao_amd import _lib
    from ao_amd.ptv2 import transform as T
    from oracle import ptv2_ref
    from tests import tester_cases as TC

    dev = "cuda"
    cfg = dict(ptv2.S3DIS_BACKBONE, drop_path_rate=0.0)
    model = ptv2.DefaultSegmentor(backbone=ptv2.PointTransformerV2(**cfg)).to(dev)
    model.backbone.load_state_dict(ptv2_ref.init_state(cfg, seed=5), strict=True)
    model.eval()
    room = TC.synthetic_room(args.points, seed=11)
    n = int(room["coord"].shape[0])
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in room.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frag = T.test_fragments(data, TC.S3DIS_TEST_CFG, transform=TC.S3DIS_BASE_TRANSFORM)
    torch.cuda.synchronize()
    fl = frag["fragment_list"]
    sizes = [int(f["index"].shape[0]) for f in fl]
    print(json.dumps(dict(leg="fragments", points=n, fragments=len(fl), rows_min=min(sizes), rows_max=max(sizes),
                          distinct_sizes=len(set(sizes)), build_ms=round((time.perf_counter() - t0) * 1e3, 1))), flush=True)

    os.environ.pop("AO_AMD_VOTE", None)
    res = {}
    res["literal"] = timed(lambda: TC.literal_loop(model, fl, n, 13, dev, T.point_collate)[0].max(1)[1], args.repeats, args.warmup)
    print(json.dumps(dict(leg="a literal loop", **res["literal"])), flush=True)
    for fb in (1, 2, 4, 8):
        run = lambda: ptv2.test_scene(model, fl, n, 13, fragment_batch=fb).predict()  # noqa: E731
        run()
        _lib.graph_stats(reset=True)
        run()
        torch.cuda.synchronize()
        g = _lib.graph_stats(reset=True)
        res[fb] = timed(run, args.repeats, 0)
        print(json.dumps(dict(leg="b test_scene", fragment_batch=fb, ratio_to_literal=round(res[fb]["wall_ms"] / res["literal"]["wall_ms"], 3),
                              graph=dict(scopes=g["scopes"], captures=g["instantiated"], updates=g["updated"], declined=g["declined"]),
                              **res[fb])), flush=True)

    # (c) the vote alone, per fragment, on the logits of the scene
    _, kept = TC.literal_loop(model, fl, n, 13, dev, T.point_collate)
    for c in (13, 200):
        if c == 13:
            sets, logits = [i for i, _ in kept], [x for _, x in kept]
        else:  # the same fragments with a ScanNet200-sized head
            g = torch.Generator(device=dev).manual_seed(1)
            sets, logits = [i for i, _ in kept], [torch.randn(i.shape[0], c, device=dev, generator=g) * 3 for i, _ in kept]
        for mode in ("torch", "hip"):
            def vote(mode=mode):
                if mode == "torch":
                    os.environ["AO_AMD_VOTE"] = "torch"
                else:
                    os.environ.pop("AO_AMD_VOTE", None)
                t = ptv2.VoteTable(n, c, dev)
                for idx, x in zip(sets, logits):
                    t.add(x, idx)
                return t

            r = timed(vote, args.repeats, args.warmup)
            os.environ.pop("AO_AMD_VOTE", None)
            print(json.dumps(dict(leg="c vote alone", classes=c, path=mode, fragments=len(sets),
                                  per_fragment_us=round(r["gpu_ms"] * 1e3 / len(sets), 2),
                                  per_fragment_wall_us=round(r["wall_ms"] * 1e3 / len(sets), 2), **r)), flush=True)
    print(json.dumps(dict(build=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
