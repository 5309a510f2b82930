"""SpUNet-v1m1: per-level times of each kernel form of ao_amd/csrc/spconv.hip on one synthetic scene, and one training step.

    python tools/bench_spunet.py [--voxels 100000] [--repeats 5] [--warmup 2] [--skip-model]

The scene is one synthetic room (ao_amd.synth.room_scene) voxelised at 0.04 m and cropped to --voxels voxels; its tables come
from one ao_amd.spunet.build_tables call, which is timed too.  Per level, every convolution shape the model runs there:
the forward, and forward plus backward (input gradient and weight gradient), with

    pairs      the valid (row, kappa) pairs of the table, counted on the table itself; `columns` is their mean per row
    tflops     2 * pairs * Cin * Cout per pass (forward: one pass, backward: two) over the time
    mfma_share tflops over the 157.3 TFLOP/s fp32 matrix rate of the MI355X -- work on valid pairs only: what a tile multiplies
               for rows that lack the column is not counted

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
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
                tab, n_in, n_out, k, fn = tables.nbr5, n0, n0, 5, lambda x, w: spunet.subm_conv(x, w, tables, 0, 5)
            elif form == "subm":
                tab, n_in, n_out, k = tables.nbr3[level], tables.n[level], tables.n[level], 3
                fn = lambda x, w, level=level: spunet.subm_conv(x, w, tables, level)  # noqa: E731
            elif form == "down":
                tab, n_in, n_out, k = tables.child[level], tables.n[level], tables.n[level + 1], 2
                fn = lambda x, w, level=level: spunet.down_conv(x, w, tables, level)  # noqa: E731
            else:
                tab, n_in, n_out, k = tables.child[level], tables.n[level + 1], tables.n[level], 2
                fn = lambda x, w, level=level: spunet.inverse_conv(x, w, tables, level)  # noqa: E731
            pairs = int((tab >= 0).sum())
            x = torch.randn(n_in, cin, device="cuda", requires_grad=True)
            w = (torch.randn(cout, k, k, k, cin, device="cuda") / (k ** 3 * cin) ** 0.5).requires_grad_(True)
            g = torch.randn(n_out, cout, device="cuda")
            row = dict(figure="conv", level=level, form=form, cin=cin, cout=cout, rows=tab.shape[0], pairs=pairs,
                       columns=round(pairs / max(tab.shape[0], 1), 2))
            for path in ("hip", "torch"):
                os.environ["AO_AMD_SPUNET"] = path
                with torch.no_grad():
                    fwd = timed(lambda: fn(x, w), args.repeats, args.warmup)
                both = timed(lambda: torch.autograd.grad(fn(x, w), [x, w], g), args.repeats, args.warmup)
                flops = 2.0 * pairs * cin * cout
                row[path] = dict(fwd_ms=round(fwd, 3), fwd_bwd_ms=round(both, 3),
                                 fwd_tflops=round(flops / fwd / 1e9, 2), fwd_bwd_tflops=round(3 * flops / both / 1e9, 2))
            row["fwd_mfma_share"] = round(row["hip"]["fwd_tflops"] / PEAK_TFLOPS, 4)
            row["fwd_bwd_mfma_share"] = round(row["hip"]["fwd_bwd_tflops"] / PEAK_TFLOPS, 4)
            row["torch_over_hip"] = round(row["torch"]["fwd_bwd_ms"] / row["hip"]["fwd_bwd_ms"], 2)
            print(json.dumps(row))
            del x, w, g
    if not args.skip_model:
        model = spunet.SpUNetBase(6, 13).cuda().train()
        feat = torch.cat([coord.float() * 0.04, torch.rand(n0, 3, device="cuda") * 2 - 1], 1)
        segment = torch.randint(0, 13, (n0,), device="cuda")
        batch = dict(discrete_coord=coord, feat=feat, offset=offset)

        def train_step():
            model.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(batch), segment).backward()

        row = dict(figure="spunet_step", n=n0)
        for path in ("hip", "torch"):
            os.environ["AO_AMD_SPUNET"] = path
            torch.cuda.reset_peak_memory_stats()
            row[path] = dict(ms=round(timed(train_step, args.repeats, args.warmup), 3),
                             peak_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
        row["torch_over_hip"] = round(row["torch"]["ms"] / row["hip"]["ms"], 2)
        print(json.dumps(row))
    print(json.dumps(dict(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0),
                          voxels=n0, numpy=np.__version__, torch=torch.__version__)))


if __name__ == "__main__":
    main()
