"""GPU: the fused per-point augmentation (ao_amd/csrc/augment.hip through ao_amd/ptv2/transform.py).

* device against the fixture of the reference's own transform.py (tests/golden/augment.npz), with the recorded noise supplied:
  colour bit-equal, coord bit-equal where no rotation precedes, else within 1 fp32 ulp and at most 0.1 % of the entries
  differing; an elastic step within max(4 elastic_ref_err, 1 fp32 ulp) -- the bounds tests/test_augment_host.py holds the
  numpy restatement to.  The two train prefixes also at n in {1, 63, 64, 65, 257}, against the restatement (bit-equal).
* Compose(fuse=True) bit-equal to the same classes called one by one with the same draws.
* the in-kernel Philox / Box-Muller normals: indexed by point, a function of the seed, within 16 fp32 ulp at 5.77 (7.6e-6) of
  the float64 restatement, standard at n = 600 001, where the grid-stride loop takes a second trip.
* bounds == torch.min / torch.max exactly; every blur pass BIT-EQUAL to the scipy-made fixture planes; one point-kernel
  launch per segment.
"""
import json

import numpy as np
import pytest
import torch

from tests import augment_cases as C
from tests import augment_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from ao_amd.ptv2 import transform

    return transform


@pytest.fixture(scope="module")
def fx():
    return C.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_maker(seed, tensor):
    return lambda dims: tensor(np.random.default_rng(seed).normal(size=tuple(dims) + (3,)).astype(np.float32))


def cut(draws, n, full, tensor):
    """the recorded draws for the first n points: noise rows sliced; below the full cloud the elastic grids are made for
    whatever size the sub-cloud's bounding box gives"""
    out = []
    for i, d in enumerate(draws):
        d = dict(d)
        if d.get("noise") is not None:
            d["noise"] = d["noise"][:n]
        if d.get("grids") is not None and n < full:
            d["grids"] = [grid_maker(1000 + 10 * i + k, tensor) for k in range(len(d["grids"]))]
        out.append(d)
    return out


def run_device(T, cfg, draws, coord, color, seed=0):
    comp = T.Compose(cfg, fuse=True)
    d = comp(dict(coord=dev(coord), color=dev(color)), draws=dict(seed=seed, per=draws))
    torch.cuda.synchronize()
    return d["coord"].cpu().numpy(), d["color"].cpu().numpy()


def test_every_case_against_the_fixture(T, fx):
    worst = 0.0
    for tag in json.loads(str(fx["cases"])):
        cfg, draws = C.case(fx, tag, tensor=dev)
        coord, color = run_device(T, cfg, draws, fx["coord"], fx["color"])
        assert coord.dtype == np.float32
        elastic = any(c["type"] == "ElasticDistortion" and d["gate"] < 0.95 for c, d in zip(cfg, draws))
        differing = C.check_against_fixture(fx, tag, coord, color, elastic)
        if elastic:
            worst = max(worst, float(np.abs(coord.astype(np.float64) - fx[tag + "_coord"].astype(np.float32)).max()))
        print("%s: %d coordinate entries differ from the fixture" % (tag, differing))
    print("elastic cases: max |device - fixture| = %.3e (elastic_ref_err %.3e)" % (worst, float(fx["elastic_ref_err"])))


def test_single_calls_return_the_reference_dtype(T, fx):
    for tag in ("rotate_z_on", "rotate_x_on", "clip", "jitter", "elastic_on", "cjitter_on"):
        cfg, draws = C.case(fx, tag, tensor=dev)
        d = T.build_transform(cfg[0])(dict(coord=dev(fx["coord"]), color=dev(fx["color"])), **draws[0])
        want = fx[tag + "_coord"]
        assert str(d["coord"].dtype).endswith(str(want.dtype)), tag
        have = d["coord"].cpu().numpy()
        if tag.startswith("rotate"):
            assert (np.abs(have - want) <= C.ulp32(want)).all()
        elif tag == "elastic_on":
            assert (np.abs(have.astype(np.float64) - want) <= np.maximum(4 * float(fx["elastic_ref_err"]), C.ulp32(want))).all()
        else:
            assert np.array_equal(have, want), tag
        assert np.array_equal(d["color"].cpu().numpy(), fx[tag + "_color"]), tag


@pytest.mark.parametrize("tag", ["s3dis_prefix", "scannet_prefix"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_prefixes_at_small_sizes(T, fx, tag, n):
    full = fx["coord"].shape[0]
    cfg, draws_d = C.case(fx, tag, tensor=dev)
    _, draws_h = C.case(fx, tag)
    coord, color = fx["coord"][:n], fx["color"][:n]
    have_coord, have_color = run_device(T, cfg, cut(draws_d, n, full, dev), coord, color)
    comp = T.Compose(cfg, fuse=True)
    segs, = comp.plan(dict(seed=0, per=cut(draws_h, n, full, np.asarray)))
    with np.errstate(all="ignore"):  # (one point: the auto-contrast divides by a zero range, as the reference would)
        want_coord, want_color = R.run_plan(segs, coord, color, elastic_grid=T.elastic_grid)
    assert np.array_equal(have_color, want_color, equal_nan=True)
    if tag == "s3dis_prefix":
        assert np.array_equal(have_coord, want_coord)
    else:  # (the restatement's own bound against the reference, tests/test_augment_host.py)
        assert (np.abs(have_coord.astype(np.float64) - want_coord) <= C.ulp32(want_coord)).all()


@pytest.mark.parametrize("tag", ["s3dis_prefix", "scannet_prefix"])
def test_fused_equals_single_calls(T, fx, tag):
    cfg, draws = C.case(fx, tag, tensor=dev)
    for d in draws:  # in-kernel noise for the jitters, given grids for the elastic pairs
        if "noise" in d:
            d["noise"] = None
    seed = 987654321987
    fused_coord, fused_color = run_device(T, cfg, draws, fx["coord"], fx["color"], seed=seed)
    d = dict(coord=dev(fx["coord"]), color=dev(fx["color"]))
    for i, (c, dr) in enumerate(zip(cfg, draws)):
        t = T.build_transform(c)
        if isinstance(t, T._PointTransform):
            d = t(d, seed=seed, stream=T._STREAMS * i, **dr)
        else:  # CenterShift, RandomScale, RandomFlip: the classes as they were
            d = t(d, **dr) if dr else t(d)
    assert np.array_equal(d["coord"].float().cpu().numpy(), fused_coord)
    assert np.array_equal(d["color"].cpu().numpy(), fused_color)
    assert not np.array_equal(fused_coord, fx["coord"]) and not np.array_equal(fused_color, fx["color"])


def noise(n, seed, stream):
    from ao_amd import _lib

    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().aug_noise_hip_launcher(n, seed, stream, out.data_ptr(), _lib.stream_ptr()), "aug_noise_hip_launcher")
    return out


def test_in_kernel_noise(T):
    big, seed = 600001, 0x1234567890ABCDEF
    g = noise(big, seed, 5)
    assert torch.equal(noise(65, seed, 5), g[:65]) and torch.equal(noise(5000, seed, 5)[:65], g[:65])  # by point, not lane
    assert torch.equal(noise(5000, seed, 5), g[:5000])
    assert not torch.equal(noise(5000, seed + 1, 5), g[:5000]) and not torch.equal(noise(5000, seed, 6), g[:5000])
    g64 = g.double().cpu().numpy()
    err = float(np.abs(g64 - R.normals64(big, seed, 5)).max())
    print("in-kernel normals: max |device - float64 restatement| = %.3e over %d values (bound 7.6e-6), max |g| %.3f"
          % (err, 3 * big, np.abs(g64).max()))
    assert err <= 16 * 2.0 ** -21  # 16 fp32 ulp at 5.77 = 7.6e-6
    for col in g64.T:  # 5 standard errors of the mean and of the variance of a standard normal
        assert abs(col.mean()) < 5 / np.sqrt(big) and abs(col.var() - 1) < 5 * np.sqrt(2 / big)
    # a scale + jitter + colour program at 600 001 points: the in-kernel noise is the noise launcher's, bit for bit
    gen = torch.Generator().manual_seed(3)
    coord = (torch.rand(big, 3, generator=gen) * 8 - 4).cuda()
    color = torch.randint(0, 256, (big, 3), generator=gen).float().cuda()
    cfg = [dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomJitter", sigma=0.01, clip=0.02),
           dict(type="ChromaticTranslation", p=1, ratio=0.05), dict(type="ChromaticJitter", p=1, std=0.05)]
    comp = T.Compose(cfg, fuse=True)
    draws = [dict(scale=[1.0625]), dict(noise=None), dict(gate=0.0, uniform=[0.25, 0.5, 0.75]), dict(gate=0.0, noise=None)]
    own = comp(dict(coord=coord, color=color), draws=dict(seed=seed, per=draws))
    fed = [dict(d) for d in draws]
    fed[1]["noise"], fed[3]["noise"] = noise(big, seed, T._STREAMS * 1), noise(big, seed, T._STREAMS * 3)
    given = comp(dict(coord=coord, color=color), draws=dict(seed=seed, per=fed))
    assert torch.equal(own["coord"], given["coord"]) and torch.equal(own["color"], given["color"])
    segs, = comp.plan(dict(seed=seed, per=[dict(d, noise=d["noise"].cpu().numpy()) if d.get("noise") is not None else d for d in fed]))
    want_coord, want_color = R.run_plan(segs, coord.cpu().numpy(), color.cpu().numpy())
    assert np.array_equal(own["coord"].cpu().numpy(), want_coord) and np.array_equal(own["color"].cpu().numpy(), want_color)
    scaled = (coord.double() * 1.0625).float().double()
    jitter = own["coord"].double() - scaled
    assert float(jitter.abs().max()) <= 0.02 + 2.0 ** -22  # |jitter| <= clip before the sum's rounding (half an ulp at 4.25)
    only = comp.transforms[1](dict(coord=torch.zeros(big, 3, device="cuda")), seed=seed, stream=8)["coord"]
    assert float(only.abs().max()) == float(np.float32(0.02)) and float((only.abs() == np.float32(0.02)).float().mean()) > 0.03


def test_bounds_are_exact(T):
    gen = torch.Generator().manual_seed(5)
    for n in (1, 64, 65, 70001):
        coord = (torch.randn(n, 3, generator=gen) * 50 - 20).cuda()
        color = torch.randint(0, 256, (n, 3), generator=gen).float().cuda()
        for c in (coord, coord.double() * 1.0000001, -coord.abs() - 1):
            b = T.aug_bounds(c, color)[:12]
            want = torch.cat([c.min(0)[0].double(), c.max(0)[0].double(), color.min(0)[0].double(), color.max(0)[0].double()])
            assert torch.equal(b, want), n
        assert torch.equal(T.aug_bounds(coord)[:6], torch.cat([coord.min(0)[0], coord.max(0)[0]]).double())


def test_blur_passes_are_bit_equal_to_scipy(T, fx):
    from ao_amd import _lib

    a = dev(fx["blur_in"])
    dims = a.shape[:3]
    for i in range(6):
        b = torch.empty_like(a)
        _lib.check(_lib.lib().aug_blur3_hip_launcher(dims[0], dims[1], dims[2], i % 3, a.data_ptr(), b.data_ptr(), _lib.stream_ptr()),
                   "aug_blur3_hip_launcher")
        assert np.array_equal(b.cpu().numpy(), fx["blur_pass%d" % i]), i
        a = b


def test_one_point_kernel_launch_per_segment(T, fx):
    from ao_amd import _lib

    for tag, launches in (("s3dis_prefix", 1), ("scannet_prefix", 5)):
        cfg, draws = C.case(fx, tag, tensor=dev)
        _lib.kernel_timer(True)
        try:
            run_device(T, cfg, draws, fx["coord"], fx["color"])
            seen = _lib.kernel_timer_read()
        finally:
            _lib.kernel_timer(False)
        assert seen["aug_points_kernel"]["launches"] == launches, (tag, seen)


def test_full_train_list_runs_on_device(T, fx):
    """raw scan -> collated batch: the S3DIS train list end to end, fused, nothing point-sized through the host"""
    cfg = json.loads(str(fx["s3dis_prefix_cfg"])) + [
        dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="train", keys=("coord", "color", "segment"), return_discrete_coord=True),
        dict(type="SphereCrop", point_max=200, mode="random"), dict(type="CenterShift", apply_z=False), dict(type="NormalizeColor"),
        dict(type="ShufflePoint"), dict(type="ToTensor"),
        dict(type="Collect", keys=("coord", "discrete_coord", "segment"), feat_keys=["coord", "color"])]
    comp = T.Compose(cfg, fuse=True, generator=torch.Generator().manual_seed(2))
    scenes = []
    for _ in range(2):
        segment = torch.arange(fx["coord"].shape[0]).cuda()
        scenes.append(comp(dict(coord=dev(fx["coord"]), color=dev(fx["color"]), segment=segment)))
    batch = T.point_collate(scenes, mix_prob=1.0, generator=torch.Generator().manual_seed(0))
    n = batch["coord"].shape[0]
    assert batch["coord"].is_cuda and batch["feat"].shape == (n, 6) and batch["offset"].tolist() == [n] and n <= 400
    assert batch["feat"][:, 3:].abs().max() <= 1 and torch.isfinite(batch["feat"]).all()
