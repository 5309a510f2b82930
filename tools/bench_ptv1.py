"""Point Transformer V1: the vector-attention layer and the Seg50 training step, HIP against AO_AMD_PTV1=torch.

    python tools/bench_ptv1.py [--points 80000] [--repeats 5] [--warmup 2] [--skip-model]

Layer: forward plus backward of ao_amd.ptv1.vector_attention (inputs x_q, x_k, x_v; everything between the q / k / v Linears
and bn2) at the five S3DIS level shapes of a scene of --points points: n = points, / 4, / 16, / 64, / 256 with (C, ns) =
(32, 8), (64, 16), (128, 16), (256, 16), (512, 16), on both paths, with the peak of the allocator over the call.  The level
clouds are farthest-point samples of one synthetic room, the neighbour tables its self-kNN; table and inverse table are made
once, outside the figure.

Model: one training step (forward, cross-entropy, backward) of PointTransformer-Seg50 on the same scene on both paths, and on
the HIP path the time spent inside pointops.farthest_point_sampling, inside pointops.knn_query and inside the attention layers
(host clock around each call with a device synchronise on both sides, in a separate instrumented step).

The host clock around calls that end in a device synchronise.  One JSON line per figure; the last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEVELS = ((32, 8), (64, 16), (128, 16), (256, 16), (512, 16))


def timed(fn, repeats, warmup):
    import torch

    for _ in range(warmup):
        fn()
    wall = []
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(wall), 3), min=round(min(wall), 3), max=round(max(wall), 3),
                peak_mb=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib, pointops, ptv1, synth
    from ao_amd.ptv1 import attention
    from ao_amd.ptv2 import gva

    torch.manual_seed(0)
    coord = torch.from_numpy(synth.room_scene(seed=0, room=0, point_max=args.points)).cuda()
    n0 = coord.shape[0]
    offset = torch.tensor([n0], dtype=torch.int32, device="cuda")
    p, o = coord, offset
    for level, (c, ns) in enumerate(LEVELS):
        if level:
            n_o = torch.tensor([p.shape[0] // 4], dtype=torch.int32, device="cuda")
            t = timed(lambda: pointops.farthest_point_sampling(p, o, n_o), 1, 0)
            print(json.dumps(dict(figure="fps", n=p.shape[0], m=int(n_o[0]), **t)))
            p, o = p[pointops.farthest_point_sampling(p, o, n_o).long()].contiguous(), n_o
        n = p.shape[0]
        idx = pointops.knn_query(ns, p, o)[0].contiguous()
        gva.inverse_table(idx)
        layer = ptv1.PointTransformerLayer(c, c, 8, ns).cuda().train()
        x = [torch.randn(n, c, device="cuda", requires_grad=True) for _ in range(3)]
        g = torch.randn(n, c, device="cuda")
        params = attention._params(layer.linear_p, layer.linear_w)

        def step():
            out = ptv1.vector_attention(*x, p, idx, layer.linear_p, layer.linear_w)
            torch.autograd.grad(out, x + params, g)

        row = dict(figure="layer", n=n, c=c, ns=ns)
        for path in ("hip", "torch"):
            os.environ["AO_AMD_PTV1"] = path
            row[path] = timed(step, args.repeats, args.warmup)
        row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row))
        del layer, x, g
    if not args.skip_model:
        model = ptv1.PointTransformerSeg50(in_channels=6, num_classes=13).cuda().train()
        feat = torch.cat([coord, torch.rand(n0, 3, device="cuda") * 2 - 1], 1)
        segment = torch.randint(0, 13, (n0,), device="cuda")
        batch = dict(coord=coord, feat=feat, offset=offset)

        def train_step():
            model.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(batch), segment).backward()

        row = dict(figure="seg50_step", n=n0)
        for path in ("hip", "torch"):
            os.environ["AO_AMD_PTV1"] = path
            row[path] = timed(train_step, args.repeats, args.warmup)
        row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row))
        # the share of FPS, kNN and the attention layers: an instrumented step on the HIP path (every bracket synchronises, so
        # its total is above the plain step; the attention's backward is bracketed through the autograd node)
        os.environ["AO_AMD_PTV1"] = "hip"
        spent = dict(fps=0.0, knn=0.0, attention_fwd=0.0, attention_bwd=0.0)

        def bracket(fn, key):
            def wrapped(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                spent[key] += (time.perf_counter() - t0) * 1e3
                return out
            return wrapped

        real = (pointops.farthest_point_sampling, pointops.knn_query, attention._VectorAttention.forward,
                attention._VectorAttention.backward)
        pointops.farthest_point_sampling = bracket(real[0], "fps")
        pointops.knn_query = bracket(real[1], "knn")
        attention._VectorAttention.forward = staticmethod(bracket(real[2], "attention_fwd"))
        attention._VectorAttention.backward = staticmethod(bracket(real[3], "attention_bwd"))
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_step()
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
        finally:
            pointops.farthest_point_sampling, pointops.knn_query = real[:2]
            attention._VectorAttention.forward, attention._VectorAttention.backward = staticmethod(real[2]), staticmethod(real[3])
        print(json.dumps(dict(figure="seg50_shares", n=n0, instrumented_step_ms=round(total, 3),
                              **{k: round(v, 3) for k, v in spent.items()},
                              **{k + "_share": round(v / total, 3) for k, v in spent.items()})))
    print(json.dumps(dict(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0),
                          points=n0, numpy=np.__version__, torch=torch.__version__)))


if __name__ == "__main__":
    main()
