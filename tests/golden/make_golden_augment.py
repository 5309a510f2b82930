"""tests/golden/make_golden_augment.py -- tests/golden/augment.npz: what the reference's training augmentations compute,
produced by RUNNING the reference's own pointcept/datasets/transform.py, unmodified, on the CPU (numpy >= 2, scipy 1.15).
Nothing here is read at test time except the file it writes.

Every draw is seeded and recorded: `random.random`, `np.random.rand`, `np.random.uniform` and `np.random.randn` are wrapped for
the duration of a case; the wrapper of randn returns fp32-representable values (the device takes its supplied normals as
fp32), so the device and the numpy restatement (tests/augment_ref.py) receive exactly the noise the reference used.  A case
is a list of transform configs run one by one on one cloud; per transform, the recorded draws are stored in the form the
classes of ao_amd.ptv2.transform take them (`<case>_draws`, JSON; arrays by npz key).

Cases: each class alone with its gate forced on and forced off, the S3DIS `sam-final` train prefix and the ScanNet base train
prefix (configs/s3dis/semseg-pt-v2m2-0-sam-final.py:71-86, configs/scannet/semseg-pt-v2m2-0-base.py:85-101 without
RandomDropout; seeds chosen so that the gates of interest are on).  Also recorded: the six scipy blur passes of one noise
grid, and `elastic_ref_err`, the distance of the reference's own elastic displacement (evaluated on a float64 copy of the
cloud) from a float64 numpy evaluation of the same smoothed grid.

usage:  python tests/golden/make_golden_augment.py <reference root>
"""
import importlib
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import augment_ref as R  # noqa: E402
from tests import tester_cases as TC  # noqa: E402

LOG = []
FORCE_RANDOM = [None]


def load_reference(ref):
    for name, sub in (("pointcept", "pointcept"), ("pointcept.utils", "pointcept/utils"), ("pointcept.datasets", "pointcept/datasets")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, sub)]
        sys.modules[name] = m
    T = importlib.import_module("pointcept.datasets.transform")
    assert T.__file__.startswith(ref), T.__file__
    return T


def wrap_rng():
    o_random, o_rand, o_uniform, o_randn = random.random, np.random.rand, np.random.uniform, np.random.randn

    def w_random():
        v = o_random() if FORCE_RANDOM[0] is None else FORCE_RANDOM[0]
        LOG.append(("random", v))
        return v

    def w_rand(*shape):
        v = o_rand(*shape)
        LOG.append(("rand", v))
        return v

    def w_uniform(*a, **k):
        v = o_uniform(*a, **k)
        LOG.append(("uniform", v))
        return v

    def w_randn(*shape):
        v = o_randn(*shape).astype(np.float32).astype(np.float64)
        LOG.append(("randn", v.copy()))  # (ChromaticJitter scales its noise in place)
        return v

    random.random, np.random.rand, np.random.uniform, np.random.randn = w_random, w_rand, w_uniform, w_randn


def draws_of(kind, log, out, tag):
    """the recorded calls of one transform -> the keyword draws of the ao_amd class"""
    def keep(name, v):
        out["%s_%s" % (tag, name)] = np.asarray(v, np.float32)
        return {"npz": "%s_%s" % (tag, name)}

    vals = [v for _, v in log]
    if kind in ("RandomRotate",):
        return dict(gate=vals[0], angle=float(vals[1]) if len(vals) > 1 else None)
    if kind == "RandomScale":
        return dict(scale=[float(v) for v in np.atleast_1d(vals[0])])
    if kind == "RandomFlip":
        return dict(draws=[float(vals[0]), float(vals[1])])
    if kind == "RandomShift":
        return dict(shift=[float(v) for v in vals])
    if kind == "RandomJitter":
        return dict(noise=keep("noise", vals[0]))
    if kind == "ElasticDistortion":
        return dict(gate=vals[0], grids=[keep("grid%d" % i, v) for i, v in enumerate(vals[1:])] or None)
    if kind == "ChromaticAutoContrast":
        return dict(gate=float(vals[0]), blend=float(vals[1]) if len(vals) > 1 else None)
    if kind == "ChromaticTranslation":
        return dict(gate=float(vals[0]), uniform=[float(v) for v in vals[1].reshape(-1)] if len(vals) > 1 else None)
    if kind == "ChromaticJitter":
        return dict(gate=float(vals[0]), noise=keep("noise", vals[1]) if len(vals) > 1 else None)
    if kind == "RandomColorDrop":
        return dict(gate=float(vals[0]))
    assert not vals, (kind, log)
    return {}


def run_case(T, out, tag, cfg, coord, color, seed, force=None, need=None):
    """runs cfg transform by transform; returns the list of draws; need(draws) -> bool picks the seed"""
    for s in range(seed, seed + 4000):
        random.seed(s)
        np.random.seed(s)
        FORCE_RANDOM[0] = force
        d = dict(coord=coord.copy(), color=color.copy())
        draws, extra = [], {}
        for i, c in enumerate(cfg):
            del LOG[:]
            d = T.TRANSFORMS.build(dict(c))(d)
            draws.append(draws_of(c["type"], list(LOG), extra, "%s_t%d" % (tag, i)))
        FORCE_RANDOM[0] = None
        if need is None or need(draws):
            break
    else:
        raise AssertionError("no seed gives the wanted gates for " + tag)
    out.update(extra)
    out[tag + "_cfg"], out[tag + "_draws"] = json.dumps(cfg), json.dumps(draws)
    out[tag + "_coord"], out[tag + "_color"] = d["coord"], d["color"]
    print("%-28s seed %4d coord %s color %s" % (tag, s, d["coord"].dtype, d["color"].dtype))
    return draws


ELASTIC = dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]])  # (the reference's default pairs, named)
S3DIS_PREFIX = [dict(type="CenterShift", apply_z=True), dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5),
                dict(type="RandomJitter", sigma=0.005, clip=0.02), dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None),
                dict(type="ChromaticTranslation", p=0.95, ratio=0.05), dict(type="ChromaticJitter", p=0.95, std=0.05)]
SCANNET_PREFIX = [dict(type="CenterShift", apply_z=True),
                  dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0.5),
                  dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=0.5),
                  dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=0.5),
                  dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=0.5),
                  dict(type="RandomJitter", sigma=0.005, clip=0.02),
                  dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]),
                  dict(type="ChromaticAutoContrast", p=0.2, blend_factor=None),
                  dict(type="ChromaticTranslation", p=0.95, ratio=0.05), dict(type="ChromaticJitter", p=0.95, std=0.05)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("POINTCEPT_ROOT", "")
    assert os.path.isdir(os.path.join(ref, "pointcept")), "usage: make_golden_augment.py <reference root>"
    T = load_reference(os.path.abspath(ref))
    import scipy.ndimage

    wrap_rng()
    out = {}
    room = TC.synthetic_room(300, seed=11)
    c = room["coord"].numpy().astype(np.float64)
    c = (c - c.min(0)) / (c.max(0) - c.min(0)) * np.array([1.5, 1.1, 0.7]) + np.array([2.25, -3.5, 0.125])
    coord, color = np.ascontiguousarray(c, np.float32), room["color"].numpy().copy()
    out["coord"], out["color"] = coord, color
    lo = coord.min(0).astype(np.float64)

    singles = [
        ("rotate_z_on", [dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True)]),
        ("rotate_z_off", [dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=0)]),
        ("rotate_x_on", [dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=1)]),
        ("rotate_y_given_on", [dict(type="RandomRotate", angle=[-0.5, 0.5], axis="y", center=[0.5, -0.25, 1.0], p=1)]),
        ("shift", [dict(type="RandomShift", shift=[[-0.2, 0.2], [-0.2, 0.2], [0, 0]])]),
        ("clip", [dict(type="PointClip", point_cloud_range=[float(lo[0]) + 0.2, float(lo[1]) + 0.2, float(lo[2]) + 0.1,
                                                            float(lo[0]) + 1.2, float(lo[1]) + 0.9, float(lo[2]) + 0.5])]),
        ("jitter", [dict(type="RandomJitter", sigma=0.005, clip=0.02)]),
        ("jitter_clipping", [dict(type="RandomJitter", sigma=0.02, clip=0.02)]),
        ("contrast_on", [dict(type="ChromaticAutoContrast", p=1, blend_factor=None)]),
        ("contrast_given_on", [dict(type="ChromaticAutoContrast", p=1, blend_factor=0.3)]),
        ("contrast_off", [dict(type="ChromaticAutoContrast", p=0, blend_factor=None)]),
        ("translation_on", [dict(type="ChromaticTranslation", p=1, ratio=0.05)]),
        ("translation_off", [dict(type="ChromaticTranslation", p=0, ratio=0.05)]),
        ("cjitter_on", [dict(type="ChromaticJitter", p=1, std=0.05)]),
        ("cjitter_off", [dict(type="ChromaticJitter", p=0, std=0.05)]),
        ("drop_on", [dict(type="RandomColorDrop", p=1, color_augment=0.3)]),
        ("drop_off", [dict(type="RandomColorDrop", p=0, color_augment=0.3)]),
    ]
    for i, (tag, cfg) in enumerate(singles):
        run_case(T, out, tag, cfg, coord, color, seed=100 + i)
    run_case(T, out, "elastic_on", [ELASTIC], coord, color, seed=200, force=0.5)
    run_case(T, out, "elastic_off", [ELASTIC], coord, color, seed=201, force=0.99)
    # an elastic step on a float64 array (after a rotation)
    run_case(T, out, "rotate_elastic", [dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], always_apply=True),
                                        ELASTIC], coord, color, seed=202, force=0.5)
    run_case(T, out, "s3dis_prefix", S3DIS_PREFIX, coord, color, seed=300,
             need=lambda d: min(d[2]["draws"]) < 0.5 and d[4]["gate"] < 0.2 and d[5]["gate"] < 0.95 and d[6]["gate"] < 0.95)
    FORCE_RANDOM[0] = None
    run_case(T, out, "scannet_prefix", SCANNET_PREFIX, coord, color, seed=400,
             need=lambda d: all(d[i]["gate"] <= 0.5 for i in (1, 2, 3)) and d[7]["gate"] < 0.95 and d[8]["gate"] < 0.2
             and d[9]["gate"] < 0.95 and d[10]["gate"] < 0.95)
    names = [k[:-4] for k in out if k.endswith("_cfg")]
    out["cases"] = json.dumps(names)

    # the six blur passes of scipy, on the first grid of the elastic case
    grid = out["elastic_on_t0_grid0"]
    out["blur_in"] = grid
    for i, shape in enumerate([(3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)] * 2):
        grid = scipy.ndimage.convolve(grid, np.ones(shape).astype("float32") / 3, mode="constant", cval=0)
        out["blur_pass%d" % i] = grid
        mine = R.blur3(out["blur_pass%d" % (i - 1)] if i else out["blur_in"], i % 3)
        print("blur pass %d: restatement bit-equal to scipy: %s" % (i, np.array_equal(mine, grid)))

    # elastic_ref_err: the reference's displacement on a float64 copy against a float64 evaluation of the same grid
    from ao_amd.ptv2.transform import elastic_grid  # (host-only helper: the grid's size and axes)
    err, c64 = 0.0, coord.astype(np.float64)
    for k, (g, m) in enumerate([[0.2, 0.4], [0.8, 1.6]]):
        np.random.seed(500 + k)
        del LOG[:]
        moved = T.ElasticDistortion.elastic_distortion(c64.copy(), g, m)
        noise = [v for n, v in LOG if n == "randn"][0].astype(np.float32)
        dims, start, spacing = elastic_grid(c64.min(0), c64.max(0), False, g)
        assert tuple(dims) + (3,) == noise.shape
        mine = R.trilinear(R.blurred(noise), c64, start, spacing) * m
        err = max(err, float(np.abs((moved - c64) - mine).max()))
        print("elastic pair %d: grid %s, max |displacement| %.3e, reference vs float64 evaluation %.3e" % (k, dims, np.abs(mine).max(), err))
        c64 = moved
    out["elastic_ref_err"] = np.float64(err)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
