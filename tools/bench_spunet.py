"""SpUNet-v1m1: per-level times of each kernel form of ao_amd/csrc/spconv.hip on one synthetic scene, and one training step.

    python tools/bench_spunet.py [--voxels 100000] [--repeats 5] [--warmup 2] [--skip-model] [--operands fp32|bf16|both]

The scene is one synthetic room (ao_amd.synth.room_scene) voxelised at 0.04 m and cropped to --voxels voxels; its tables come
from one ao_amd.spunet.build_tables call, which is timed too.  Per level, every convolution shape the model runs there:
the forward, and forward plus backward (input gradient and weight gradient), with

    pairs      the valid (row, kappa) pairs of the table, counted on the table itself; `columns` is their mean per row
    tflops     2 * pairs * Cin * Cout per pass (forward: one pass, backward: two) over the time
    mfma_share tflops over the 157.3 TFLOP/s fp32 matrix rate of the MI355X -- work on valid pairs only: what a tile multiplies
               for rows that lack the column is not counted

--operands both (the A/B of ao_amd/csrc/spconv_bf16.hip) times every matrix-core row and the step with fp32 and with bf16
operands in alternation -- fp32, bf16, fp32, bf16, ... for --repeats rounds after a warm-up of both -- and reports each one's
median under "hip" and "hip_bf16" with bf16_over_fp32 = bf16 time / fp32 time (forward + backward); the eager path is then
left out.  mfma_share stays relative to the fp32 matrix rate in every column.

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

PEAK_TFLOPS = 157.3
# (form, Cin, Cout) per level of SpUNetBase's default channels; "down" leaves the level, "inverse" arrives at it
SHAPES = (
    (("stem", 6, 32), ("subm", 128, 96), ("subm", 96, 96), ("down", 32, 32), ("inverse", 96, 96)),
    (("subm", 32, 32), ("subm", 128, 96), ("subm", 96, 96), ("down", 32, 64), ("inverse", 128, 96)),
    (("subm", 64, 64), ("subm", 192, 128), ("subm", 128, 128), ("down", 64, 128), ("inverse", 256, 128)),
    (("subm", 128, 128), ("subm", 384, 256), ("subm", 256, 256), ("down", 128, 256), ("inverse", 256, 256)),
    (("subm", 256, 256),),
)


def timed(fn, repeats, warmup):
    import torch

    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall)


def alternated(fns, repeats, warmup):
    """medians of several callables timed in alternation: one round calls each once"""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    wall = [[] for _ in fns]
    for _ in range(repeats):
        for at, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[at].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(w) for w in wall]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--operands", choices=("fp32", "bf16", "both"), default="fp32")
    args = ap.parse_args()
    import numpy as np
    import torch

    from ao_amd import _lib, spunet, synth

    torch.manual_seed(0)
    pts = synth.room_scene(seed=0, room=1, point_max=args.voxels)
    vox = np.floor((pts - pts.min(0)) / 0.04).astype(np.int64)
    _, first = np.unique(vox, axis=0, return_index=True)
    coord = torch.from_numpy(vox[np.sort(first)].astype(np.int32)).cuda()
    n0 = coord.shape[0]
    offset = torch.tensor([n0], dtype=torch.int32, device="cuda")
    ms = timed(lambda: spunet.build_tables(coord, offset), args.repeats, args.warmup)
    tables = spunet.build_tables(coord, offset)
    print(json.dumps(dict(figure="tables", n=tables.n, ms=round(ms, 3))))
    for level, shapes in enumerate(SHAPES):
        for form, cin, cout in shapes:
            if form == "stem":
                tab, n_in, n_out, k, fn = tables.nbr5, n0, n0, 5, lambda x, w, ops="fp32": spunet.subm_conv(x, w, tables, 0, 5, ops)
            elif form == "subm":
                tab, n_in, n_out, k = tables.nbr3[level], tables.n[level], tables.n[level], 3
                fn = lambda x, w, ops="fp32", level=level: spunet.subm_conv(x, w, tables, level, operands=ops)  # noqa: E731
            elif form == "down":
                tab, n_in, n_out, k = tables.child[level], tables.n[level], tables.n[level + 1], 2
                fn = lambda x, w, ops="fp32", level=level: spunet.down_conv(x, w, tables, level, ops)  # noqa: E731
            else:
                tab, n_in, n_out, k = tables.child[level], tables.n[level + 1], tables.n[level], 2
                fn = lambda x, w, ops="fp32", level=level: spunet.inverse_conv(x, w, tables, level, ops)  # noqa: E731
            pairs = int((tab >= 0).sum())
            x = torch.randn(n_in, cin, device="cuda", requires_grad=True)
            w = (torch.randn(cout, k, k, k, cin, device="cuda") / (k ** 3 * cin) ** 0.5).requires_grad_(True)
            g = torch.randn(n_out, cout, device="cuda")
            row = dict(figure="conv", level=level, form=form, cin=cin, cout=cout, rows=tab.shape[0], pairs=pairs,
                       columns=round(pairs / max(tab.shape[0], 1), 2))
            flops = 2.0 * pairs * cin * cout

            def figures(fwd, both):
                return dict(fwd_ms=round(fwd, 3), fwd_bwd_ms=round(both, 3), fwd_tflops=round(flops / fwd / 1e9, 2),
                            fwd_bwd_tflops=round(3 * flops / both / 1e9, 2))

            if args.operands == "both":
                if form == "stem":
                    continue  # (no bf16 form)
                os.environ["AO_AMD_SPUNET"] = "hip"
                kinds = ("fp32", "bf16")
                with torch.no_grad():
                    fwd = alternated([lambda ops=ops: fn(x, w, ops) for ops in kinds], args.repeats, args.warmup)
                both = alternated([lambda ops=ops: torch.autograd.grad(fn(x, w, ops), [x, w], g) for ops in kinds], args.repeats, args.warmup)
                row["hip"], row["hip_bf16"] = figures(fwd[0], both[0]), figures(fwd[1], both[1])
                row["fwd_mfma_share"] = round(row["hip"]["fwd_tflops"] / PEAK_TFLOPS, 4)
                row["bf16_over_fp32"] = dict(fwd=round(fwd[1] / fwd[0], 3), fwd_bwd=round(both[1] / both[0], 3))
                print(json.dumps(row))
                del x, w, g
                continue
            for path in ("hip", "torch"):
                os.environ["AO_AMD_SPUNET"] = path
                with torch.no_grad():
                    fwd = timed(lambda: fn(x, w, args.operands), args.repeats, args.warmup)
                both = timed(lambda: torch.autograd.grad(fn(x, w, args.operands), [x, w], g), args.repeats, args.warmup)
                row[path] = figures(fwd, both)
            row["operands"] = args.operands
            row["fwd_mfma_share"] = round(row["hip"]["fwd_tflops"] / PEAK_TFLOPS, 4)
            row["fwd_bwd_mfma_share"] = round(row["hip"]["fwd_bwd_tflops"] / PEAK_TFLOPS, 4)
            row["torch_over_hip"] = round(row["torch"]["fwd_bwd_ms"] / row["hip"]["fwd_bwd_ms"], 2)
            print(json.dumps(row))
            del x, w, g
    if not args.skip_model:
        models = {ops: spunet.SpUNetBase(6, 13, conv_operands=ops).cuda().train()
                  for ops in (("fp32", "bf16") if args.operands == "both" else (args.operands,))}
        feat = torch.cat([coord.float() * 0.04, torch.rand(n0, 3, device="cuda") * 2 - 1], 1)
        segment = torch.randint(0, 13, (n0,), device="cuda")
        batch = dict(discrete_coord=coord, feat=feat, offset=offset)

        def train_step(model):
            model.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(batch), segment).backward()

        row = dict(figure="spunet_step", n=n0, operands=args.operands)
        if args.operands == "both":
            os.environ["AO_AMD_SPUNET"] = "hip"
            ms = alternated([lambda m=m: train_step(m) for m in models.values()], args.repeats, args.warmup)
            row.update(hip=dict(ms=round(ms[0], 3)), hip_bf16=dict(ms=round(ms[1], 3)), bf16_over_fp32=round(ms[1] / ms[0], 3))
        else:
            for path in ("hip", "torch"):
                os.environ["AO_AMD_SPUNET"] = path
                torch.cuda.reset_peak_memory_stats()
                row[path] = dict(ms=round(timed(lambda: train_step(models[args.operands]), args.repeats, args.warmup), 3),
                                 peak_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
            row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row))
    print(json.dumps(dict(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0),
                          voxels=n0, numpy=np.__version__, torch=torch.__version__)))


if __name__ == "__main__":
    main()
