"""CPU: the host side of Masked Scene Contrast (ao_amd/msc, include/ptv2_msc_hip.h): the numpy restatement
against the reference's recorded run, the state dict, the header's binding, the registry, the two MSC transform lists and the
refusals of RandomColorJitter."""
import json
import os

import numpy as np
import pytest
import torch

from tests import msc_ref as R
from tests.msc_cases import GOLDEN, configs, fixture, heads64, knn_of, model_kwargs


@pytest.mark.parametrize("prefix,rate,t", [("a.", 0.4, 0.4), ("b.", 0.0, 0.07)])
def test_ref_reproduces_the_fixture(prefix, rate, t):
    """tests/msc_ref.py on the fixture's inputs and the reference's draws gives what the reference's forward recorded: masks and
    pairs exactly, the float64 losses to 1e-12 of themselves when fed the rows the reference gathered -- which leaves the
    recorded fp32 values within a few fp32 roundings"""
    fix = fixture()
    o1, f1, o2, f2 = fix["view1_origin_coord"], fix["view1_offset"], fix["view2_origin_coord"], fix["view2_offset"]
    assert o1.shape[1] == 3 and len(f1) == len(f2) == 2 and o1.min() < 0, "centred scenes: negative cells"
    mask1, mask2 = R.cross_masks(o1, f1, o2, f2, 0.1, rate, fix[prefix + "mask_perm"])
    assert np.array_equal(mask1, fix[prefix + "mask1"]) and np.array_equal(mask2, fix[prefix + "mask2"])
    assert len(fix[prefix + "mask_perm"]) == R.patch_count(o1, f1, o2, f2, 0.1)
    idx, d2 = knn_of(fix)
    radius = float(fix["radius"])
    d = np.sqrt(d2[idx >= 0].astype(np.float64))
    assert np.abs(d - radius).min() / radius > 1e-4, "every distance keeps its margin from the radius"
    counts = R.hit_counts(idx, d2, radius)
    assert {0, 1, 2} <= set(counts.tolist()), "rows without a hit, with one and with several"
    draws = R.spread_draws(idx, d2, radius, fix[prefix + "match_draws"])
    pairs = R.match(idx, d2, radius, draws)
    cut = prefix == "a."
    assert (len(fix[prefix + "pair_perm"]) == len(pairs)) == cut
    pairs = R.cut_pairs(pairs, int(fix["a.max_pair"]) if cut else 8192, fix[prefix + "pair_perm"])
    assert np.array_equal(pairs, fix[prefix + "match_index"])
    # the losses, from the rows the reference gathered
    want = R.info_nce(fix["view1_out"], fix["view2_out"], pairs, t)
    again = R.info_nce(fix["view1_out"][pairs[:, 0]], fix["view2_out"][pairs[:, 1]], np.stack([np.arange(len(pairs))] * 2, 1), t)
    for key in ("loss", "pos_sim", "neg_sim"):
        assert abs(want[key] - again[key]) <= 1e-12 * abs(want[key])
    total = want["loss"]
    for key, name in (("loss", "nce_loss"), ("pos_sim", "pos_sim"), ("neg_sim", "neg_sim")):
        have = float(fix[prefix + "result." + name])
        assert abs(have - want[key]) <= 4e-6 * max(abs(want[key]), 1e-1), (name, have, want[key])
    if cut:
        c = R.color_loss(heads64(fix, prefix, "color_head", fix["view1_out"], mask1), fix["view1_color"][mask1],
                         heads64(fix, prefix, "color_head", fix["view2_out"], mask2), fix["view2_color"][mask2])
        n = R.normal_loss(heads64(fix, prefix, "normal_head", fix["view1_out"], mask1), fix["view1_normal"][mask1],
                          heads64(fix, prefix, "normal_head", fix["view2_out"], mask2), fix["view2_normal"][mask2])
        assert abs(float(fix["a.result.color_loss"]) - c) <= 4e-6 * abs(c)
        assert abs(float(fix["a.result.normal_loss"]) - n) <= 4e-6  # (a mean of dot products of unit vectors, near zero)
        total = total + c + n
    else:
        assert sorted(k for k in fix if k.startswith("b.result.")) == ["b.result.loss", "b.result.nce_loss", "b.result.neg_sim", "b.result.pos_sim"]
    assert abs(float(fix[prefix + "result.loss"]) - total) <= 4e-6 * abs(total)


def test_voxel_grid_aliasing_in_the_restatement():
    """ids are not shifted to zero: cell (-1, 1, 0) and cell (nx - 1, 0, 0) share an id when nx cells span x"""
    origin = np.array([[-0.05, 0.15, 0.05], [0.25, 0.05, 0.05], [0.05, 0.05, 0.05]], np.float32)  # cells (-1,1,0) (2,0,0) (0,0,0)
    offset = np.array([3], np.int32)
    none = np.zeros((0, 3), np.float32)
    ids = R.patch_ids(origin, offset, none, np.array([0], np.int32), 0.1)
    assert ids.tolist() == [2, 2, 0]
    assert len(set(R.alias_free_ids(origin, offset, none, np.array([0], np.int32), 0.1).tolist())) == 3


def test_manifest_and_state_dict():
    from ao_amd import msc, spunet

    with open(os.path.join(GOLDEN, "msc_manifest.json")) as f:
        manifest = json.load(f)
    recorded = configs()
    backbone = recorded["base"]["model"]["backbone"]
    assert recorded["base"]["model"]["type"] == recorded["pointcontrast"]["model"]["type"] == "MSC-v1m1"
    both = [msc.MaskedSceneContrast(**model_kwargs(recorded[name])) for name in ("base", "pointcontrast")]
    assert (both[0].nce_t, both[0].mask_rate, both[0].view1_mix_prob, both[0].normal_head) == (0.4, 0.4, 0.8, None)
    assert (both[1].nce_t, both[1].mask_rate, both[1].matching_max_pair, both[1].color_head) == (0.07, 0, 4096, None)
    assert both[1].mask_token.shape == (1, 3)
    for name, heads in (("heads", True), ("no_heads", False)):
        model = msc.MaskedSceneContrast(backbone=dict(backbone), backbone_in_channels=6, backbone_out_channels=96,
                                        reconstruct_color=heads, reconstruct_normal=heads)
        have = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert have == manifest[name] and list(have) == list(manifest[name]), "the reference's keys in the reference's order"
        assert isinstance(model.backbone, spunet.SpUNetBase) and model.backbone.num_classes == 0
        rest = [k for k in have if not k.startswith("backbone.")]
        assert rest == (["mask_token", "color_head.weight", "color_head.bias", "normal_head.weight", "normal_head.bias"] if heads
                        else ["mask_token"])
    token = model.mask_token.detach()
    assert token.shape == (1, 6) and 0 < float(token.abs().max()) <= 2.0 and model.mask_token.requires_grad  # trunc_normal_(std=0.02), cut at +-2
    # the reference's defaults
    assert (model.mask_grid_size, model.mask_rate, model.view1_mix_prob, model.view2_mix_prob, model.matching_max_k,
            model.matching_max_radius, model.matching_max_pair, model.nce_t, model.contrast_weight, model.reconstruct_weight) == \
        (0.1, 0.4, 0, 0, 8, 0.03, 8192, 0.4, 1, 1)
    given = torch.nn.Linear(3, 4)
    assert msc.MaskedSceneContrast(backbone=given, backbone_in_channels=3, backbone_out_channels=4).backbone is given


def test_header_binding_and_registry():
    from ao_amd import _abi
    from ao_amd.ptv2 import registry

    assert _abi.msc_consts == dict(MSC_MAX_PAIRS=16384, MSC_MAX_CHANNELS=256, MSC_MAX_K=64)
    assert sorted(_abi.msc_signatures) == ["msc_match_hip_launcher", "msc_nce_bwd_hip_launcher", "msc_nce_fwd_hip_launcher",
                                           "msc_patch_ids_hip_launcher", "ptv2_msc_abi_version", "ptv2_msc_nce_workspace_bytes"]
    assert len(_abi.msc_signatures["msc_nce_fwd_hip_launcher"][1]) == 17 and len(_abi.msc_signatures["msc_nce_bwd_hip_launcher"][1]) == 17

    class Registry(dict):
        def register_module(self, module, name, force=False):
            self[name] = module

    models = Registry()
    done = registry.register(MODELS=models)
    from ao_amd.msc import MaskedSceneContrast

    assert models["MSC-v1m1"] is MaskedSceneContrast and "MSC-v1m1" not in done


def test_library_refusals():
    """sizes are checked before any launch: no GPU is needed to be refused"""
    from ao_amd import _lib

    L = _lib.lib()
    assert L.ptv2_msc_abi_version() == 1
    assert L.ptv2_msc_nce_workspace_bytes(4096, 96) < 16 << 20, "about ten (M, C) arrays"
    assert L.ptv2_msc_nce_workspace_bytes(0, 96) == -1 and L.ptv2_msc_nce_workspace_bytes(16385, 96) == -1
    assert L.ptv2_msc_nce_workspace_bytes(64, 6) == -1 and L.ptv2_msc_nce_workspace_bytes(64, 260) == -1
    p = 4096  # (never dereferenced: every call below is refused)
    assert L.msc_nce_fwd_hip_launcher(8, 8, 0, 96, p, p, p, 0.4, p, p, p, p, p, p, p, 1 << 30, 0) == 1
    assert L.msc_nce_fwd_hip_launcher(8, 8, 8, 6, p, p, p, 0.4, p, p, p, p, p, p, p, 1 << 30, 0) == 1
    assert L.msc_nce_fwd_hip_launcher(8, 8, 8, 96, p, p, p, 0.0, p, p, p, p, p, p, p, 1 << 30, 0) == 1
    assert L.msc_nce_fwd_hip_launcher(8, 8, 8, 96, p, p, p, 0.4, p, p, p, p, p, p, p, 16, 0) == 2
    assert L.msc_nce_bwd_hip_launcher(8, 8, 8, 96, p, p, 0.4, p, p, p, p, p, p, p, p, 16, 0) == 2
    assert L.msc_match_hip_launcher(8, 65, 8, p, p, p, 0.03, p, 0) == 1
    assert L.msc_patch_ids_hip_launcher(8, 8, 0, p, p, p, p, 0.1, p, p, 0) == 1
    assert L.msc_patch_ids_hip_launcher(8, 8, 1, p, p, p, p, 0.0, p, p, 0) == 1


def test_ops_refusals_on_the_host():
    from ao_amd import msc

    one = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="mask_rate"):
        msc.cross_masks(torch.zeros(4, 3), one, torch.zeros(4, 3), one, 0.1, 0.6)
    with pytest.raises(RuntimeError, match="GPU only"):
        msc.info_nce(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros((2, 2), dtype=torch.int64), 0.4)


def test_both_transform_lists_build():
    from ao_amd.ptv2 import transform as T

    g = torch.Generator().manual_seed(1)
    recorded = configs()
    BASE_TRANSFORM, VIEW_TRANS = recorded["base"]["transform"], recorded["base"]["transform"][3]["view_trans_cfg"]
    assert recorded["pointcontrast"]["view1_transform"] == recorded["pointcontrast"]["view2_transform"]
    assert [c["type"] for c in VIEW_TRANS].count("RandomColorJitter") == 1 and BASE_TRANSFORM[3]["type"] == "ContrastiveViewsGenerator"
    for cfg in (BASE_TRANSFORM, recorded["pointcontrast"]["view1_transform"]):
        for fuse in (False, True):
            pipe = T.Compose(cfg, fuse=fuse, generator=g)
            assert [type(t).__name__ for t in pipe.transforms] == [c["type"] for c in cfg]
    views = T.Compose(BASE_TRANSFORM, fuse=True, generator=g).transforms[3]
    assert isinstance(views, T.ContrastiveViewsGenerator) and views.view_trans.fuse and views.view_trans.generator is g
    assert [type(t).__name__ for t in views.view_trans.transforms] == [c["type"] for c in VIEW_TRANS]
    assert not T.Compose(BASE_TRANSFORM).transforms[3].view_trans.fuse
    assert "RandomColorJitter" not in T.__doc__.split("Not here, on purpose")[1].split("\n\n")[0]


def test_color_jitter_checks():
    from ao_amd.ptv2.transform import RandomColorJitter as J

    j = J(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.02, p=0.8)
    assert j.brightness == [0.6, 1.4] and j.contrast == [0.6, 1.4] and j.saturation == [0.8, 1.2] and j.hue == [-0.02, 0.02] and j.p == 0.8
    d = J()
    assert d.brightness is None and d.contrast is None and d.saturation is None and d.hue is None and d.p == 0.95
    assert J(brightness=2).brightness == [0.0, 3.0], "the lower end is cut at zero"
    assert J(brightness=(1.0, 1.0)).brightness is None and J(hue=(0.0, 0.0)).hue is None
    for kwargs in (dict(brightness=-0.1), dict(hue=-0.1), dict(hue=(-0.6, 0.1)), dict(contrast=(2.0, 1.0)), dict(saturation=(-1.0, 1.0))):
        with pytest.raises(ValueError):
            J(**kwargs)
    for kwargs in (dict(brightness="a"), dict(hue=(0.1, 0.2, 0.3)), dict(contrast=None)):
        with pytest.raises(TypeError):
            J(**kwargs)
    color = torch.rand(5, 3) * 255
    for name, bad in (("brightness", -1.0), ("contrast", -1.0), ("saturation", -1.0), ("hue", 0.6), ("hue", -0.6)):
        with pytest.raises(ValueError):
            getattr(j, "adjust_" + name)(color, bad)


def test_color_jitter_draw_order():
    """get_params: the order first, then the factors of the adjustments that are switched on; a gate per adjustment reached"""
    from ao_amd.ptv2.transform import RandomColorJitter as J

    g = torch.Generator().manual_seed(3)
    order = torch.randperm(4, generator=g).tolist()
    b = 0.6 + 0.8 * float(torch.rand((), dtype=torch.float64, generator=g))
    h = -0.02 + 0.04 * float(torch.rand((), dtype=torch.float64, generator=g))
    got = J(brightness=0.4, hue=0.02).get_params(torch.Generator().manual_seed(3))
    assert got[0] == order and got[1][1] is None and got[1][2] is None
    assert abs(got[1][0] - b) < 1e-15 and abs(got[1][3] - h) < 1e-15
    # gates above p: nothing changes
    color = torch.rand(7, 3) * 255
    out = J(brightness=0.4, hue=0.02, p=0.5)(dict(color=color.clone()), draws=dict(order=order, factors=got[1], gates=[0.9] * 4))
    assert torch.equal(out["color"], color)


def test_color_jitter_matches_numpy_on_the_host():
    """the same tensor operations on CPU tensors: brightness, saturation and hue equal the recorded numpy run bit for bit, the
    contrast differs by the order of its one mean (the GPU form of this test is tests/test_gpu_msc_transform.py)"""
    from ao_amd.ptv2.transform import RandomColorJitter as J

    fix = fixture()
    j = J(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.02, p=0.8)
    color = torch.from_numpy(fix["cj.color"])
    seen = 0
    for key in fix:
        if not key.startswith("cj.") or key.count(".") < 2 or key.startswith("cj.full"):
            continue
        _, name, factor = key.split(".", 2)
        got = getattr(j, "adjust_" + name)(color.clone(), float(factor)).numpy()
        assert got.dtype == np.float32
        if name == "contrast":
            assert np.abs(got - fix[key]).max() <= 255 * 2.0 ** -20
        else:
            assert np.array_equal(got, fix[key]), key
        seen += 1
    assert seen == 9
