"""GPU: the two transforms Masked Scene Contrast adds to ao_amd/ptv2/transform.py.  ContrastiveViewsGenerator over the transform list
of configs/scannet/pretrain-msc-v1m1-0-spunet-base.py; RandomColorJitter against a recorded numpy run of the reference
(tests/golden/msc.npz, cj.*): brightness, saturation and hue bit for bit; contrast through its one reduction, the mean of the gray
values, which is held to the M-rule against float64 (numpy's pairwise fp32 mean in the place of the eager error) -- the blend
around it is bit-equal given that mean."""
import numpy as np
import pytest
import torch

from tests.msc_cases import FLOOR, M_TOL_MEAN, configs, fixture

pytestmark = pytest.mark.gpu


def scene(n=6000, seed=0):
    from ao_amd import synth

    rng = np.random.default_rng(seed)
    normal = rng.normal(0, 1, (n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return dict(coord=torch.from_numpy(synth.room_cloud(n, seed=seed)).float().cuda(),
                color=torch.from_numpy(rng.uniform(0, 255, (n, 3)).astype(np.float32)).cuda(),
                normal=torch.from_numpy(normal.astype(np.float32)).cuda())


@pytest.mark.parametrize("fuse", [False, True])
def test_contrastive_views_over_the_config_list(fuse):
    from ao_amd.ptv2 import transform as T

    torch.manual_seed(3)
    pipe = T.Compose(configs()["base"]["transform"], fuse=fuse, generator=torch.Generator().manual_seed(1),
                     device_generator=torch.Generator(device="cuda").manual_seed(2))
    head = T.Compose(pipe.transforms[:3], fuse=fuse, generator=pipe.generator)
    data = head(scene())
    origin = data["origin_coord"].float().cpu().numpy()
    for t in pipe.transforms[3:]:
        data = t(data)
    keys = ["view%d_%s" % (v, k) for v in (1, 2) for k in ("origin_coord", "discrete_coord", "coord", "color", "normal", "offset", "feat")]
    assert sorted(data) == sorted(keys)
    known = {row.tobytes() for row in origin}
    for v in (1, 2):
        n = data["view%d_coord" % v].shape[0]
        assert 500 < n < origin.shape[0] and data["view%d_offset" % v].tolist() == [n]
        assert data["view%d_feat" % v].shape == (n, 6) and data["view%d_feat" % v].dtype == torch.float32
        assert all(data["view%d_%s" % (v, k)].shape == (n, 3) for k in ("origin_coord", "discrete_coord", "color", "normal"))
        assert all(row.tobytes() in known for row in data["view%d_origin_coord" % v].float().cpu().numpy()), "rows of the input's"
        dc = data["view%d_discrete_coord" % v]
        assert not dc.is_floating_point() and int(dc.min()) >= 0
        assert float(data["view%d_color" % v].abs().max()) <= 1.0 + 1e-6  # NormalizeColor
    o1, o2 = data["view1_origin_coord"], data["view2_origin_coord"]
    assert o1.shape != o2.shape or not torch.equal(o1, o2), "successive draws: the two views differ"
    assert not torch.equal(data["view1_coord"][:100], data["view2_coord"][:100])


def test_color_jitter_against_the_recorded_numpy_run():
    from ao_amd.ptv2.transform import RandomColorJitter as J

    fix = fixture()
    j = J(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.02, p=0.8)
    color = torch.from_numpy(fix["cj.color"]).cuda()
    seen = 0
    for key in fix:
        if not key.startswith("cj.") or key.count(".") < 2 or key.startswith("cj.full"):
            continue
        _, name, factor = key.split(".", 2)
        got = getattr(j, "adjust_" + name)(color.clone(), float(factor))
        assert got.dtype == torch.float32 and got.is_cuda
        if name == "contrast":
            check_contrast(j, color, float(factor), got.cpu().numpy(), fix[key])
        else:
            assert np.array_equal(got.cpu().numpy(), fix[key]), key
        seen += 1
    assert seen == 9


def check_contrast(j, color, factor, got, recorded):
    gray = j.rgb_to_grayscale(color)
    mean = gray.mean().cpu().numpy()
    gray = gray.cpu().numpy()
    exact = gray.astype(np.float64).mean()
    e_kernel, e_numpy = abs(float(mean) - exact) / exact, abs(float(np.mean(gray)) - exact) / exact
    print("msc color jitter contrast %.2f: mean of gray, device %.3e numpy %.3e ratio %.2f" % (factor, e_kernel, e_numpy, e_kernel / max(e_numpy, FLOOR)))
    assert e_kernel <= M_TOL_MEAN * max(e_numpy, FLOOR)
    c = color.cpu().numpy()
    blend = lambda m: (factor * c + (1.0 - factor) * np.float32(m)).clip(0, 255.0).astype(np.float32)  # noqa: E731
    assert np.array_equal(got, blend(mean)), "the reference's blend around the device's mean"
    assert np.array_equal(recorded, blend(np.mean(gray))), "and around numpy's in the recorded run"


def test_color_jitter_whole_call_with_recorded_draws():
    from ao_amd.ptv2.transform import RandomColorJitter as J

    fix = fixture()
    j = J(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.02, p=0.8)
    draws = dict(order=fix["cj.full.order"].tolist(), factors=fix["cj.full.factors"].tolist(), gates=fix["cj.full.gates"].tolist())
    got = j(dict(color=torch.from_numpy(fix["cj.color"]).cuda()), draws=draws)["color"].cpu().numpy()
    applied = [fn for at, fn in enumerate(draws["order"]) if draws["gates"][at] < 0.8]
    assert len(applied) >= 2, "the recorded call applies several adjustments"
    if 1 in applied:  # contrast among them: one rounding of its mean may move a value by an ulp, and later steps carry that on
        assert np.abs(got - fix["cj.full"]).max() <= 255 * 2.0 ** -20
    else:
        assert np.array_equal(got, fix["cj.full"])
    # from a generator: the same call twice with the same seed
    a = j(dict(color=torch.from_numpy(fix["cj.color"]).cuda()), generator=torch.Generator().manual_seed(4))["color"]
    b = j(dict(color=torch.from_numpy(fix["cj.color"]).cuda()), generator=torch.Generator().manual_seed(4))["color"]
    assert torch.equal(a, b) and not torch.equal(a.cpu(), torch.from_numpy(fix["cj.color"]))
