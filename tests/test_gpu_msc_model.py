"""GPU: MaskedSceneContrast (ao_amd/msc/model.py) against the reference's recorded run (tests/golden/msc.npz) and over a small real
SpUNetBase, on both paths (HIP and AO_AMD_MSC=torch).

Recorded run: the model gets the recorded backbone outputs, state and draws; masks and pairs are exact, and every returned entry
is held to the M-rule of tests/test_gpu_msc_ops.py against float64 (tests/msc_ref.py), with the recorded fp32 CPU value in the
place of the eager error.  Real backbone: the narrowest widths the sparse-convolution kernels take are multiples of 32, so the
backbone is channels = (32,) * 8 with one block per stage."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import msc_ref as R
from tests.msc_cases import FLOOR, M_TOL, M_TOL_EAGER, M_TOL_PATHS, fixture, heads64, knn_of

pytestmark = pytest.mark.gpu


class Recorded(nn.Module):
    def __init__(self, feats):
        super().__init__()
        self.feats, self.calls, self.offsets = feats, 0, []

    def forward(self, data_dict):
        self.calls += 1
        self.offsets.append(data_dict["offset"].clone())
        return self.feats[(self.calls - 1) % 2]


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("prefix", ["a.", "b."])
def test_recorded_run(prefix, path, monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    fix = fixture()
    heads = prefix == "a."
    feats = [torch.from_numpy(fix["view%d_out" % v]).cuda().requires_grad_(True) for v in (1, 2)]
    model = msc.MaskedSceneContrast(
        backbone=Recorded(feats), backbone_in_channels=6, backbone_out_channels=16, matching_max_k=int(fix["max_k"]),
        matching_max_radius=float(fix["radius"]), mask_rate=0.4 if heads else 0, nce_t=0.4 if heads else 0.07,
        matching_max_pair=int(fix["a.max_pair"]) if heads else 8192, reconstruct_color=heads, reconstruct_normal=heads).cuda().train()
    state = {k[len(prefix + "state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith(prefix + "state.")}
    assert model.load_state_dict(state, strict=True)
    idx, d2 = knn_of(fix)
    draws = dict(mask_perm=torch.from_numpy(fix[prefix + "mask_perm"]),
                 row_draws=torch.from_numpy(R.spread_draws(idx, d2, float(fix["radius"]), fix[prefix + "match_draws"])),
                 pair_perm=torch.from_numpy(fix[prefix + "pair_perm"]) if heads else None)
    batch = {k: torch.from_numpy(v).cuda() for k, v in fix.items() if k.startswith("view") and not k.endswith("_out")}
    seen = {}
    masks, match = model.generate_cross_masks, model.match_contrastive_pair
    model.generate_cross_masks = lambda *a, **k: seen.setdefault("masks", masks(*a, **k))
    model.match_contrastive_pair = lambda *a, **k: seen.setdefault("pairs", match(*a, **k))
    res = model(batch, draws=draws)
    mask1, mask2 = (m.cpu().numpy() for m in seen["masks"])
    pairs = seen["pairs"].cpu().numpy()
    assert np.array_equal(mask1, fix[prefix + "mask1"]) and np.array_equal(mask2, fix[prefix + "mask2"])
    assert np.array_equal(pairs, fix[prefix + "match_index"])
    assert sorted(res) == sorted(k[len(prefix + "result."):] for k in fix if k.startswith(prefix + "result."))
    assert res["loss"].requires_grad and not res["pos_sim"].requires_grad and not res["neg_sim"].requires_grad

    t = model.nce_t
    ref = R.info_nce(fix["view1_out"], fix["view2_out"], pairs, t)
    want = dict(nce_loss=ref["loss"], pos_sim=ref["pos_sim"], neg_sim=ref["neg_sim"], loss=ref["loss"])
    scale = dict(nce_loss=abs(ref["pos_sim"]) / t, pos_sim=0.0, neg_sim=abs(ref["pos_sim"]) / len(pairs), loss=abs(ref["pos_sim"]) / t)
    tol = dict(nce_loss=M_TOL["loss"], pos_sim=M_TOL["pos_sim"], neg_sim=M_TOL["neg_sim"], loss=max(M_TOL["loss"], M_TOL_EAGER))
    if heads:
        p = [heads64(fix, prefix, name, fix["view%d_out" % v], m) for name in ("color_head", "normal_head") for v, m in ((1, mask1), (2, mask2))]
        want["color_loss"] = R.color_loss(p[0], fix["view1_color"][mask1], p[1], fix["view2_color"][mask2])
        want["normal_loss"] = R.normal_loss(p[2], fix["view1_normal"][mask1], p[3], fix["view2_normal"][mask2])
        unit = [q / (np.linalg.norm(q, axis=1, keepdims=True) + 1e-10) for q in p[2:]]
        # (a mean of dot products of both signs: measured against the mean of their magnitudes)
        scale["normal_loss"] = (np.abs(unit[0] * fix["view1_normal"][mask1]).sum() + np.abs(unit[1] * fix["view2_normal"][mask2]).sum()) / (
            len(unit[0]) + len(unit[1]))
        scale["color_loss"] = 0.0
        tol["color_loss"] = tol["normal_loss"] = M_TOL_EAGER
        want["loss"] = want["loss"] + want["color_loss"] + want["normal_loss"]
    for key, value in want.items():
        denom = max(abs(value), scale[key])
        e_got = abs(float(res[key].detach()) - value) / denom
        e_rec = abs(float(fix[prefix + "result." + key]) - value) / denom
        print("msc recorded %s%-11s %s got %.3e recorded %.3e ratio %.2f" % (prefix, key, path, e_got, e_rec, e_got / max(e_rec, FLOOR)))
        assert e_got <= tol[key] * max(e_rec, FLOOR), (key, float(res[key]), value, e_got, e_rec)
    res["loss"].backward()
    named = np.zeros(len(fix["view1_out"]), bool)
    named[pairs[:, 0]] = True
    named |= mask1 if heads else False
    g = feats[0].grad.cpu().numpy()
    assert g[named].any(1).all() and not g[~named].any(), "a gradient for exactly the rows a pair or a mask names"


def small_batch(seed, shift_second=40, n=600):
    """two scenes of about n voxels per view on a 0.02 m lattice of 26^3 cells; the second scene's voxels lie `shift_second`
    cells along x from the first's: mixing the two then puts no two rows on one voxel, unless the shift is 0"""
    rng = np.random.default_rng(seed)
    out = {1: [], 2: []}
    side = 26
    for scene in range(2):
        cells = rng.permutation(side ** 3)[:int(n * 1.25)]
        voxel = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1)
        color = rng.uniform(-1, 1, (len(voxel), 3)).astype(np.float32)
        normal = rng.normal(0, 1, (len(voxel), 3))
        normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
        for view in (1, 2):
            keep = np.sort(rng.permutation(len(voxel))[:n + 7 * view + scene])
            v = voxel[keep].copy()
            origin = ((v + 0.5) * 0.02 - side * 0.01 + rng.uniform(-0.004, 0.004, v.shape)).astype(np.float32)
            v[:, 0] += shift_second * scene
            out[view].append(dict(origin=origin, voxel=v.astype(np.int32), color=color[keep], normal=normal[keep]))
    batch = {}
    for view in (1, 2):
        cat = lambda k: np.concatenate([s[k] for s in out[view]])  # noqa: E731
        shared = len(np.unique(cat("voxel"), axis=0)) < len(cat("voxel"))
        assert shared == (shift_second == 0), "two scenes share a voxel exactly when they are not moved apart"
        batch["view%d_origin_coord" % view] = cat("origin")
        batch["view%d_coord" % view] = cat("origin") * np.float32(1.02)
        batch["view%d_discrete_coord" % view] = cat("voxel")
        batch["view%d_color" % view], batch["view%d_normal" % view] = cat("color"), cat("normal")
        batch["view%d_feat" % view] = np.concatenate([cat("color"), cat("normal")], 1)
        batch["view%d_offset" % view] = np.cumsum([len(s["origin"]) for s in out[view]]).astype(np.int32)
    return {k: torch.from_numpy(v).cuda() for k, v in batch.items()}


def small_model(seed=0):
    from ao_amd import msc

    torch.manual_seed(seed)
    backbone = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32,) * 8, layers=(1,) * 8)
    return msc.MaskedSceneContrast(backbone=backbone, backbone_in_channels=6, backbone_out_channels=32, matching_max_radius=0.03,
                                   matching_max_pair=512).cuda().train()


def run_small(model, batch, path, monkeypatch, mix=(False, False)):
    monkeypatch.setenv("AO_AMD_MSC", path)
    model.zero_grad(set_to_none=True)
    from ao_amd import msc

    draws = {}
    n = len(torch.unique(msc.patch_ids(batch["view1_origin_coord"], batch["view1_offset"], batch["view2_origin_coord"],
                                       batch["view2_offset"], model.mask_grid_size)))
    draws["mask_perm"] = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    draws["row_draws"] = torch.randint(0, 8, (batch["view1_coord"].shape[0],), generator=torch.Generator().manual_seed(2))
    draws["pair_perm"] = None
    res = model(dict(batch), mix=mix, draws=draws)
    res["loss"].backward()
    return {k: float(v) for k, v in res.items()}, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_small_backbone_trains_on_both_paths(monkeypatch):
    model, batch = small_model(), small_batch(5)
    # more matches than matching_max_pair would need a permutation of a size known only inside: keep every pair
    model.matching_max_pair = 8192
    hip, g_hip = run_small(model, batch, "hip", monkeypatch)
    eager, g_eager = run_small(model, batch, "torch", monkeypatch)
    assert sorted(hip) == ["color_loss", "loss", "nce_loss", "neg_sim", "normal_loss", "pos_sim"]
    assert all(np.isfinite(v) for v in hip.values())
    names = [k for k, _ in model.named_parameters()]
    assert sorted(g_hip) == sorted(names), "every backbone and head parameter has a gradient"
    assert float(g_hip["mask_token"].abs().min()) > 0, "the stem's input gradient reaches the token"
    for k in names:
        assert bool(torch.isfinite(g_hip[k]).all()) and float(g_hip[k].abs().max()) > 0, k
    # The two paths differ in info_nce alone, and each is held to the M-rule against float64 in tests/test_gpu_msc_ops.py.  There
    # is no float64 run of the backbone, so here the rule is stated on the distance between the paths: at most
    # M_TOL_PATHS * 2^-24, relative to the eager value for a returned entry and in relative L2 for a parameter's gradient
    # (M_TOL_PATHS: twice the ratio measured on an MI355X, rounded up to a power of two, at most 64; tests/msc_cases.py)
    for k in ("nce_loss", "pos_sim", "neg_sim", "color_loss", "normal_loss", "loss"):
        ratio = abs(hip[k] - eager[k]) / abs(eager[k]) / FLOOR
        print("msc small model %-11s hip %.9g eager %.9g ratio %.2f" % (k, hip[k], eager[k], ratio))
    ratios = {k: float((g_hip[k] - g_eager[k]).norm() / g_eager[k].norm()) / FLOOR for k in names}
    worst = max(ratios, key=ratios.get)
    print("msc small model: parameter gradients between the paths, worst ratio %.2f (%s), median %.2f" % (
        ratios[worst], worst, float(np.median(list(ratios.values())))))
    for k in ("nce_loss", "pos_sim", "neg_sim", "color_loss", "normal_loss", "loss"):
        assert abs(hip[k] - eager[k]) <= M_TOL_PATHS[k] * FLOOR * abs(eager[k]), (k, hip[k], eager[k])
    assert ratios[worst] <= M_TOL_PATHS["grad"], (worst, ratios[worst])


def test_mixing_edits_the_offset_only(monkeypatch):
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    model, batch = small_model(), small_batch(6)
    model.matching_max_pair = 8192
    seen = []
    inner = model.backbone.forward
    model.backbone.forward = lambda d: seen.append({k: v for k, v in d.items()}) or inner(d)
    plain, _ = run_small(model, batch, "hip", monkeypatch)
    mixed, _ = run_small(model, batch, "hip", monkeypatch, mix=(True, False))
    assert all(np.isfinite(v) for v in mixed.values()) and mixed["nce_loss"] != plain["nce_loss"]
    p1, p2, m1, m2 = seen
    assert p1["offset"].tolist() == batch["view1_offset"].tolist() and m1["offset"].tolist() == batch["view1_offset"][-1:].tolist()
    assert m2["offset"].tolist() == p2["offset"].tolist() == batch["view2_offset"].tolist()
    for a, b in ((p1, m1), (p2, m2)):
        assert sorted(a) == sorted(b) == ["coord", "discrete_coord", "feat", "offset", "origin_coord"]
        for k in a:
            if k != "offset":
                assert torch.equal(a[k], b[k]), k


def test_mixing_scenes_that_share_a_voxel_raises(monkeypatch):
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    model, batch = small_model(), small_batch(7, shift_second=0)
    with torch.no_grad():
        model(dict(batch), mix=(False, False))  # unmixed: two clouds, nothing shared within one
        with pytest.raises(ValueError, match="view1_mix_prob"):
            model(dict(batch), mix=(True, False))
