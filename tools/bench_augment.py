"""tools/bench_augment.py -- the per-point train prefixes, fused against one call per class, on a synthetic raw scan.

    python tools/bench_augment.py [--points 1000000] [--repeats 30]

Prints one JSON line per prefix: median / min ms of `Compose(cfg, fuse=True)` and of the same classes called one by one with the
same draws (the classes as they were where they exist -- CenterShift, RandomScale, RandomFlip -- single-step programs otherwise),
and the point-kernel launches of the fused run.  Discipline: 5 warm-up runs of each form, then the two forms ALTERNATE run by
run (a clock ramp or a neighbour's load hits both alike), each run bracketed by torch.cuda events after a synchronize; the
median and the minimum are reported, not a mean.  The elastic pairs read their bounds back (one synchronisation each), so
their share of the time is host latency, in both forms.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ao_amd import _lib  # noqa: E402
from ao_amd.ptv2 import transform as T  # noqa: E402

S3DIS = [dict(type="CenterShift", apply_z=True), dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5),
         dict(type="RandomJitter", sigma=0.005, clip=0.02), dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None),
         dict(type="ChromaticTranslation", p=0.95, ratio=0.05), dict(type="ChromaticJitter", p=0.95, std=0.05)]
SCANNET = [dict(type="CenterShift", apply_z=True), dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5),
           dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=0.5), dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=0.5),
           dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5), dict(type="RandomJitter", sigma=0.005, clip=0.02),
           dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]), dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None),
           dict(type="ChromaticTranslation", p=0.95, ratio=0.05), dict(type="ChromaticJitter", p=0.95, std=0.05)]


def all_on(comp):
    """draws with every gate open (the worst case of the list)"""
    d = comp.draw()
    for t, dr in zip(comp.transforms, d["per"]):
        if "gate" in dr:
            dr["gate"] = 0.0
        if isinstance(t, T.RandomRotate):
            dr["angle"] = 0.3 * t.angle[1]
        if isinstance(t, T.ChromaticAutoContrast):
            dr["blend"] = 0.5
        if isinstance(t, T.ChromaticTranslation):
            dr["uniform"] = [0.25, 0.5, 0.75]
        if isinstance(t, T.RandomFlip):
            dr["draws"] = [0.0, 0.0]
    return d


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    coord = (torch.rand(args.points, 3, generator=g) * torch.tensor([12.0, 9.0, 3.0])).cuda()
    color = torch.randint(0, 256, (args.points, 3), generator=g).float().cuda()
    for name, cfg in (("s3dis", S3DIS), ("scannet", SCANNET)):
        comp = T.Compose(cfg, fuse=True, generator=torch.Generator().manual_seed(1))
        draws = all_on(comp)

        def fused():
            return comp(dict(coord=coord, color=color), draws=draws)

        def single():
            d = dict(coord=coord, color=color)
            for i, (t, dr) in enumerate(zip(comp.transforms, draws["per"])):
                if isinstance(t, T._PointTransform):
                    d = t(d, seed=draws["seed"], stream=T._STREAMS * i, **dr)
                else:
                    d = t(d, **dr) if dr else t(d)
            return d

        for _ in range(5):
            fused(), single()
        _lib.kernel_timer(True)
        fused()
        launches = _lib.kernel_timer_read()["aug_points_kernel"]["launches"]
        _lib.kernel_timer(False)
        tf, ts = [], []
        for _ in range(args.repeats):
            tf.append(timed(fused))
            ts.append(timed(single))
        print(json.dumps(dict(prefix=name, points=args.points, fused_ms_median=round(statistics.median(tf), 4), fused_ms_min=round(min(tf), 4),
                              single_ms_median=round(statistics.median(ts), 4), single_ms_min=round(min(ts), 4),
                              fused_point_launches=launches, repeats=args.repeats)))


if __name__ == "__main__":
    main()
