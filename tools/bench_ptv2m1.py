"""PT-v2m1 (GroupedLinear + position multiplier): the fused multiplier logits stage of ao_amd/csrc/gva_mul.hip against
AO_AMD_GVA=unfused (the literal op sequence) in the same build.

    python tools/bench_ptv2m1.py [--points 120000] [--repeats 5] [--warmup 2] [--no-step]

Block: one Block (pe_multiplier, GroupedLinear) forward + backward at each level of the S3DIS PT-v2m1 config
(tests/golden/ptv2m1_manifest.json: the reference config's backbone keywords) on one synthetic scene of --points points
(ao_amd.synth.scene_batch): the level's own size, coordinates and neighbour table from the model's geometry; the fifth shape
of the family, (512, 64), which only the ScanNet configs reach, runs on the coarsest of these levels.  Step: the whole
PT-v2m1 training step (DefaultSegmentor forward, backward, FlatAdamW) on that scene.  Each figure is taken fused and unfused
alternately: after --warmup calls of each, the median of --repeats calls, the host clock around work that ends in a device
synchronise; the peak is torch.cuda.max_memory_allocated over one further call, above what was allocated before it.  One JSON
line per figure, printed and appended to profiles/ptv2m1_bench.jsonl; the last carries the build digest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATHS = ("fused", "unfused")


def both(fn, repeats, warmup):
    import torch

    wall = {p: [] for p in PATHS}
    for p in PATHS:
        os.environ["AO_AMD_GVA"] = p
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        for p in PATHS:  # alternating: both see the same machine
            os.environ["AO_AMD_GVA"] = p
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[p].append((time.perf_counter() - t0) * 1e3)
    row = {}
    for p in PATHS:
        os.environ["AO_AMD_GVA"] = p
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        row[p] = dict(ms=round(statistics.median(wall[p]), 3), min_ms=round(min(wall[p]), 3), max_ms=round(max(wall[p]), 3),
                      repeats=repeats, peak_mb=round(peak / 2 ** 20, 1))
    os.environ["AO_AMD_GVA"] = "fused"
    row["unfused_over_fused"] = round(row["unfused"]["ms"] / row["fused"]["ms"], 2)
    row["peak_unfused_over_fused"] = round(row["unfused"]["peak_mb"] / max(row["fused"]["peak_mb"], 0.1), 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import torch

    from ao_amd import _lib, synth
    from ao_amd.ptv2 import Block, DefaultSegmentor, PointTransformerV2M1, gva
    from ao_amd.ptv2.model import use_grouped_linear
    from ao_amd.ptv2.optim import FlatAdamW

    if not torch.cuda.is_available():
        raise SystemExit("bench_ptv2m1: needs the GPU")
    with open(os.path.join(ROOT, "tests", "golden", "ptv2m1_manifest.json")) as f:
        cfg = json.load(f)["s3dis_cfg"]
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    torch.manual_seed(0)
    batch = {k: torch.from_numpy(v).cuda() for k, v in synth.scene_batch([0], point_max=args.points,
                                                                         in_channels=cfg["in_channels"]).items()}
    model = PointTransformerV2M1(**cfg).cuda().train()
    geo = model.geometry(batch["coord"], batch["offset"].int())
    shapes = [(cfg["patch_embed_channels"], cfg["patch_embed_groups"], cfg["dec_neighbours"][0])]
    shapes += [(c, g, k) for c, g, k in zip(cfg["enc_channels"], cfg["enc_groups"], cfg["enc_neighbours"])]
    levels = list(enumerate(shapes))
    if (512, 64, 16) not in shapes:  # the fifth shape of the family (the ScanNet configs' deepest level) on the coarsest level here
        levels.append((len(shapes) - 1, (512, 64, 16)))
    for level, (c, g, k) in levels:
        lv = geo.levels[level]
        n = lv.coord.shape[0]
        idx = lv.neighbours(k)
        blk = use_grouped_linear(Block(c, g, pe_multiplier=True, pe_bias=True)).cuda().train()
        feat = torch.randn(n, c, device="cuda").requires_grad_(True)
        gout = torch.randn(n, c, device="cuda")

        def call():
            blk.zero_grad(set_to_none=True)
            feat.grad = None
            blk([lv.coord, feat, lv.offset], idx)[1].backward(gout)

        emit(figure="block_fwd_bwd", level=level, n=n, k=k, channels=c, groups=g, nkc_tensor_mb=round(n * k * c * 4 / 2 ** 20, 1),
             fused_is_default=bool(gva.mul_supported(c, g, n, k)), **both(call, args.repeats, args.warmup))
        del blk, feat, gout
    del model, geo
    if not args.no_step:
        seg = DefaultSegmentor(dict(cfg, type="PT-v2m1")).cuda().train()
        opt = FlatAdamW(seg.parameters(), lr=0.006, weight_decay=0.05)

        def step():
            loss = seg(batch)["loss"]
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        emit(figure="train_step", config="s3dis/semseg-pt-v2m1-0-base", points=int(batch["coord"].shape[0]),
             **both(step, args.repeats, args.warmup))
    emit(figure="build", info=_lib.lib().ptv2_build_info().decode(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
         literal_shapes=[list(s) for s in gva.MUL_LITERAL_SHAPES])
    with open(os.path.join(ROOT, "profiles", "ptv2m1_bench.jsonl"), "a") as f:
        f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
