"""GPU: MaskedSceneContrastCSC (ao_amd/msc/model.py, MSC-v1m2) against the reference's recorded run (tests/golden/msc_csc.npz) and
over a small real SpUNetBase, on both paths (HIP and AO_AMD_MSC=torch).

Recorded run: the model gets the recorded backbone outputs, state and draws; the pairs are exact, and every returned entry is
held to the M-rule of tests/test_gpu_msc_csc_ops.py against float64 (tests/msc_csc_ref.py), with the recorded fp32 CPU value's
error in the place of the eager error.  Real backbone: channels = (32,) * 8 with one block per stage, 3 input channels as in the
CSC config."""
import numpy as np
import pytest
import torch

from tests import msc_csc_ref as C
from tests import msc_ref as R
from tests.msc_cases import knn_of
from tests.msc_csc_cases import FLOOR, M_TOL_PATHS, M_TOL_RECORDED, config, fixture
from tests.test_gpu_msc_model import Recorded, small_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("prefix", ["a.", "b."])
def test_recorded_run(prefix, path, monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    fix = fixture()
    cut = prefix == "a."
    r1, r2 = (float(v) for v in fix[prefix + "r"])
    feats = [torch.from_numpy(fix["view%d_out" % v]).cuda().requires_grad_(True) for v in (1, 2)]
    model = msc.MaskedSceneContrastCSC(
        backbone=Recorded(feats), backbone_in_channels=6, backbone_out_channels=16, matching_max_k=int(fix["max_k"]),
        matching_max_radius=float(fix["radius"]), mask_rate=0, nce_t=0.4, matching_max_pair=int(fix["a.max_pair"]) if cut else 8192,
        reconstruct_color=False, reconstruct_normal=False, partitions=4, r1=r1, r2=r2).cuda().train()
    state = {k[len(prefix + "state."):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith(prefix + "state.")}
    assert sorted(state) == ["mask_token"] and model.load_state_dict(state, strict=True)
    idx, d2 = knn_of(fix)
    draws = dict(mask_perm=torch.from_numpy(fix[prefix + "mask_perm"]),
                 row_draws=torch.from_numpy(R.spread_draws(idx, d2, float(fix["radius"]), fix[prefix + "match_draws"])),
                 pair_perm=torch.from_numpy(fix[prefix + "pair_perm"]) if cut else None)
    batch = {k: torch.from_numpy(v).cuda() for k, v in fix.items() if k.startswith("view") and not k.endswith("_out")}
    seen = {}
    match = model.match_contrastive_pair
    model.match_contrastive_pair = lambda *a, **k: seen.setdefault("pairs", match(*a, **k))
    res = model(batch, draws=draws)
    pairs = seen["pairs"].cpu().numpy()
    assert np.array_equal(pairs, fix[prefix + "match_index"])
    assert sorted(res) == sorted(k[len(prefix + "result."):] for k in fix if k.startswith(prefix + "result."))
    assert res["loss"].requires_grad and not res["pos_sim"].requires_grad and not res["neg_sim"].requires_grad
    assert [o.tolist() for o in model.backbone.offsets] == [fix["view1_offset"].tolist(), fix["view2_offset"].tolist()]
    # the partition the model would form eagerly is the recorded one
    scene = C.scenes_of(pairs, fix["view1_offset"], len(fix["view1_out"]))
    rows = torch.from_numpy(np.nonzero(scene == 0)[0]).cuda()
    part = model.compute_partitions(batch["view1_origin_coord"][seen["pairs"][rows, 0]], batch["view2_origin_coord"][seen["pairs"][rows, 1]])
    assert np.array_equal(part.cpu().numpy(), fix[prefix + "part.0"])

    ref = C.csc_nce(fix["view1_out"], fix["view2_out"], fix["view1_origin_coord"], fix["view2_origin_coord"], fix["view1_offset"],
                    pairs, 0.4, r1, r2)
    want = dict(nce_loss=ref["loss"], pos_sim=ref["pos_sim"], neg_sim=ref["neg_sim"], loss=ref["loss"])
    for key, value in want.items():
        e_got = abs(float(res[key].detach()) - value) / abs(value)
        e_rec = abs(float(fix[prefix + "result." + key]) - value) / abs(value)
        print("msc csc recorded %s%-8s %-5s got %.3e recorded %.3e ratio %.2f" % (prefix, key, path, e_got, e_rec, e_got / max(e_rec, FLOOR)))
        assert e_got <= M_TOL_RECORDED[key] * max(e_rec, FLOOR), (key, float(res[key]), value, e_got, e_rec)
    res["loss"].backward()
    named = np.zeros(len(fix["view1_out"]), bool)
    named[pairs[:, 0]] = True
    g = feats[0].grad.cpu().numpy()
    assert g[named].any(1).all() and not g[~named].any(), "a gradient for exactly the rows a pair names"


def small_model(seed=0, **kwargs):
    from ao_amd import msc

    torch.manual_seed(seed)
    backbone = dict(type="SpUNet-v1m1", in_channels=3, num_classes=0, channels=(32,) * 8, layers=(1,) * 8)
    cfg = dict(backbone=backbone, backbone_in_channels=3, backbone_out_channels=32, mask_rate=0, matching_max_radius=0.03,
               matching_max_pair=8192, reconstruct_color=False, reconstruct_normal=False, r1=0.125, r2=0.5)
    return msc.MaskedSceneContrastCSC(**dict(cfg, **kwargs)).cuda().train()


def run_small(model, batch, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_MSC", path)
    model.zero_grad(set_to_none=True)
    draws = dict(row_draws=torch.randint(0, 8, (batch["view1_coord"].shape[0],), generator=torch.Generator().manual_seed(2)))
    res = model(dict(batch), mix=(False, False), draws=draws)
    res["loss"].backward()
    return {k: float(v) for k, v in res.items()}, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_small_backbone_trains_on_both_paths(monkeypatch):
    """one training step over a real sparse U-Net, HIP against eager (section 13's way: there is no float64 run of the backbone,
    so the rule is stated on the distance between the paths, over 2^-24)"""
    batch = small_batch(5)
    for v in (1, 2):
        batch["view%d_feat" % v] = batch["view%d_color" % v]  # the CSC config feeds the colour alone
    model = small_model()
    hip, g_hip = run_small(model, batch, "hip", monkeypatch)
    eager, g_eager = run_small(model, batch, "torch", monkeypatch)
    assert sorted(hip) == ["loss", "nce_loss", "neg_sim", "pos_sim"]
    assert all(np.isfinite(v) for v in hip.values()) and hip["loss"] > 0
    assert sorted(g_hip) == sorted(k for k, _ in model.named_parameters()), "every parameter has a gradient"
    assert not g_hip["mask_token"].any(), "mask_rate = 0: the token weighs nothing"
    names = [k for k in g_hip if k != "mask_token"]
    for k in names:
        assert bool(torch.isfinite(g_hip[k]).all()) and float(g_hip[k].abs().max()) > 0, k
    for k in ("nce_loss", "pos_sim", "neg_sim", "loss"):
        print("msc csc small model %-8s hip %.9g eager %.9g ratio %.2f" % (k, hip[k], eager[k], abs(hip[k] - eager[k]) / abs(eager[k]) / FLOOR))
    ratios = {k: float((g_hip[k] - g_eager[k]).norm() / g_eager[k].norm()) / FLOOR for k in names}
    worst = max(ratios, key=ratios.get)
    print("msc csc small model: parameter gradients between the paths, worst ratio %.2f (%s), median %.2f" % (
        ratios[worst], worst, float(np.median(list(ratios.values())))))
    for k in ("nce_loss", "pos_sim", "neg_sim", "loss"):
        assert abs(hip[k] - eager[k]) <= M_TOL_PATHS[k] * FLOOR * abs(eager[k]), (k, hip[k], eager[k])
    assert ratios[worst] <= M_TOL_PATHS["grad"], (worst, ratios[worst])


def test_config_lists_through_pair_views(monkeypatch):
    """two frames of a synthetic room through the recorded transform lists and pair_views, collated, through the model"""
    from ao_amd import synth
    from ao_amd.ptv2 import transform as T

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    recorded = config()
    gens = dict(generator=torch.Generator().manual_seed(0), device_generator=torch.Generator(device="cuda").manual_seed(0))
    lists = [T.Compose(recorded[k], fuse=True, **gens) for k in ("view1_transform", "view2_transform")]
    scenes = []
    for room in range(2):
        rng = np.random.default_rng(room)
        cloud = torch.from_numpy(synth.room_cloud(6000, seed=room)).float().cuda()
        color = torch.from_numpy(rng.uniform(0, 255, (6000, 3)).astype(np.float32)).cuda()
        # (the same points in both frames: CenterShift then moves both alike, and the views differ by their draws alone)
        frames = [dict(coord=cloud.clone(), color=color.clone()) for _ in range(2)]
        scenes.append(T.pair_views(frames[0], frames[1], lists[0], lists[1]))
    assert sorted(scenes[0]) == sorted("view%d_%s" % (v, k) for v in (1, 2) for k in ("origin_coord", "discrete_coord", "coord", "color",
                                                                                       "offset", "feat"))
    batch = T.point_collate(scenes)
    model = small_model(matching_max_pair=512)
    res = model(batch, mix=(False, False))
    assert sorted(res) == ["loss", "nce_loss", "neg_sim", "pos_sim"] and bool(torch.isfinite(res["loss"])) and float(res["loss"]) > 0
    res["loss"].backward()
    assert max(float(p.grad.abs().max()) for p in model.backbone.parameters() if p.grad is not None) > 0
