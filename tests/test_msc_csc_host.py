"""CPU: the host side of MSC-v1m2 (CSC; ao_amd/msc, include/ptv2_csc_hip.h): the torch restatement against the
reference's recorded run, the header's binding, the registry, the state dict, the recorded config and `pair_views`."""
import json
import os

import numpy as np
import pytest
import torch

from tests import msc_csc_ref as C
from tests.msc_csc_cases import GOLDEN, config, csc_case, fixture, model_kwargs


@pytest.mark.parametrize("prefix", ["a.", "b."])
def test_ref_reproduces_the_fixture(prefix):
    """tests/msc_csc_ref.py on the recorded pairs: its classes are the reference's partition matrices exactly, every off-diagonal
    distance keeps the generator's margin from r1 and r2, and its float64 scalars leave the recorded fp32 values within a few
    fp32 roundings (the reference accumulates ten cross-entropies, each a mean over at most 250 rows, in fp32)"""
    fix = fixture()
    r1, r2 = (float(v) for v in fix[prefix + "r"])
    pairs, o1, o2, off1 = fix[prefix + "match_index"], fix["view1_origin_coord"], fix["view2_origin_coord"], fix["view1_offset"]
    scene = C.scenes_of(pairs, off1, len(o1))
    assert sorted(np.unique(scene).tolist()) == [0, 1] and len(off1) == 2
    seen = set()
    for s in (0, 1):
        rows = np.nonzero(scene == s)[0]
        x, y = o1[pairs[rows, 0]], o2[pairs[rows, 1]]
        cls = C.classes(x, y, r1, r2).numpy()
        assert np.array_equal(cls, C.recorded_to_classes(fix[prefix + "part.%d" % s]))
        off = ~np.eye(len(rows), dtype=bool)
        d = C.distances64(x, y)
        assert np.abs(d[off] - r1).min() / r1 > 1e-4 and np.abs(d[off] - r2).min() / r2 > 1e-4
        assert (np.diagonal(cls) == C.NONE).all(), "matched pairs lie below r1: the diagonal is `none`"
        seen |= set(cls[off].tolist())
    if prefix == "a.":
        assert seen == {0, 1, 2, 3, C.NONE} and len(pairs) == int(fix["a.max_pair"]) < len(fix["a.pair_perm"])
        assert (np.diff(scene) < 0).any(), "cut by the permutation: the pairs interleave the scenes"
    else:
        assert seen == {C.NONE} and (np.diff(scene) >= 0).all()
    want = C.csc_nce(fix["view1_out"], fix["view2_out"], o1, o2, off1, pairs, 0.4, r1, r2)
    for key, name in (("loss", "nce_loss"), ("loss", "loss"), ("pos_sim", "pos_sim"), ("neg_sim", "neg_sim")):
        have = float(fix[prefix + "result." + name])
        assert abs(have - want[key]) <= 4e-6 * max(abs(want[key]), 1e-1), (name, have, want[key])
    assert sorted(k for k in fix if k.startswith(prefix + "result.")) == [prefix + "result." + k for k in ("loss", "nce_loss", "neg_sim", "pos_sim")]


def test_restatement_conventions():
    """the orientation of rel, the override order and the rel_z == 0 rule on four hand-made points"""
    x = np.array([[0, 0, 0], [0, 0, 0.25], [0, 0, 1.0], [0.25, 0, 0]], np.float32)
    y = np.zeros((4, 3), np.float32)
    cls = C.classes(x, y, 0.125, 0.5).numpy()
    assert cls[0].tolist() == [C.NONE, 0, 2, C.NONE], "row i reads x_j - y_i: up near, up far, and rel_z == 0 stays none"
    assert C.classes(y, x, 0.125, 0.5).numpy()[0].tolist() == [C.NONE, C.NONE, C.NONE, C.NONE]
    assert C.classes(y, x, 0.125, 0.5).numpy()[:, 0].tolist() == [C.NONE, 1, 3, C.NONE], "the transposed partition differs"
    assert C.classes(x, y, 0.5, 0.125).numpy()[0].tolist() == [C.NONE, 2, 2, C.NONE], "r1 > r2: the first band is empty"
    case = csc_case((12, 9), c=8, seed=1)
    counts = C.class_counts(case["o1"], case["o2"], case["offset1"], case["pairs"], case["r1"], case["r2"])
    assert [c.shape for c in counts] == [(12, 5), (9, 5)] and all((c.sum(1) == len(c) - 1).all() for c in counts)


def test_header_binding_and_registry():
    from ao_amd import _abi, _lib
    from ao_amd.ptv2 import registry

    assert _abi.csc_consts == dict(CSC_MAX_PAIRS=16384, CSC_MAX_CHANNELS=256, CSC_MAX_SCENES=1024, CSC_CLASSES=5, CSC_MAX_INV_T=40)
    assert sorted(_abi.csc_signatures) == ["csc_nce_bwd_hip_launcher", "csc_nce_fwd_hip_launcher", "ptv2_csc_abi_version",
                                           "ptv2_csc_nce_workspace_bytes"]
    assert len(_abi.csc_signatures["csc_nce_fwd_hip_launcher"][1]) == 25 and len(_abi.csc_signatures["csc_nce_bwd_hip_launcher"][1]) == 23
    assert not set(_abi.csc_signatures) & set(_abi.msc_signatures) and _lib.EXPECTED_CSC_ABI == 1

    class Registry(dict):
        def register_module(self, module, name, force=False):
            self[name] = module

    models = Registry()
    done = registry.register(MODELS=models)
    from ao_amd.msc import MaskedSceneContrast, MaskedSceneContrastCSC

    assert models["MSC-v1m2"] is MaskedSceneContrastCSC and models["MSC-v1m1"] is MaskedSceneContrast and "MSC-v1m2" not in done


def test_library_refusals():
    """sizes are checked before any launch: no GPU is needed to be refused"""
    from ao_amd import _lib

    L = _lib.lib()
    assert L.ptv2_csc_abi_version() == 1
    assert 0 < L.ptv2_csc_nce_workspace_bytes(4096, 96, 1) < 16 << 20
    for m, c, b in ((0, 96, 1), (16385, 96, 1), (64, 6, 1), (64, 260, 1), (64, 96, 0), (64, 96, 1025)):
        assert L.ptv2_csc_nce_workspace_bytes(m, c, b) == -1
    p = 4096  # (never dereferenced: every call below is refused)
    fwd = lambda m, c, b, t, parts, ws: L.csc_nce_fwd_hip_launcher(  # noqa: E731
        8, 8, m, c, b, p, p, p, p, p, p, t, 0.125, 0.5, parts, p, p, p, p, p, p, p, p, ws, 0)
    assert fwd(0, 96, 1, 0.4, 4, 1 << 30) == 1 and fwd(8, 6, 1, 0.4, 4, 1 << 30) == 1 and fwd(8, 96, 0, 0.4, 4, 1 << 30) == 1
    assert fwd(8, 96, 1, 0.0, 4, 1 << 30) == 1 and fwd(8, 96, 1, 0.02, 4, 1 << 30) == 1 and fwd(8, 96, 1, 0.4, 0, 1 << 30) == 1
    assert fwd(8, 96, 1, 0.4, 4, 16) == 2
    assert L.csc_nce_bwd_hip_launcher(8, 8, 8, 96, 1, p, p, p, 0.4, 0.125, 0.5, 4, p, p, p, p, p, p, p, p, p, 16, 0) == 2
    assert L.csc_nce_bwd_hip_launcher(8, 8, 8, 96, 1, p, p, p, 0.02, 0.125, 0.5, 4, p, p, p, p, p, p, p, p, p, 1 << 30, 0) == 1


def test_manifest_state_dict_and_config():
    from ao_amd import msc, spunet
    from ao_amd.ptv2 import transform as T

    with open(os.path.join(GOLDEN, "msc_csc_manifest.json")) as f:
        manifest = json.load(f)
    recorded = config()
    assert recorded["model"]["type"] == "MSC-v1m2" and recorded["config"].endswith("pretrain-msc-v1m2-0-spunet-csc.py")
    model = msc.MaskedSceneContrastCSC(**model_kwargs(recorded))
    have = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert have == manifest["config"] and list(have) == list(manifest["config"]), "the reference's keys in the reference's order"
    assert isinstance(model.backbone, spunet.SpUNetBase) and model.backbone.num_classes == 0
    assert [k for k in have if not k.startswith("backbone.")] == ["mask_token"] and model.mask_token.shape == (1, 3)
    assert (model.partitions, model.r1, model.r2, model.mask_rate, model.nce_t, model.color_head, model.normal_head) == \
        (4, 2, 20, 0, 0.4, None, None)
    heads = msc.MaskedSceneContrastCSC(backbone=dict(recorded["model"]["backbone"], in_channels=6), backbone_in_channels=6,
                                       backbone_out_channels=96)
    have = {k: list(v.shape) for k, v in heads.state_dict().items()}
    assert have == manifest["heads"] and list(have) == list(manifest["heads"])
    # the reference's defaults
    assert (heads.mask_grid_size, heads.mask_rate, heads.view1_mix_prob, heads.view2_mix_prob, heads.matching_max_k,
            heads.matching_max_radius, heads.matching_max_pair, heads.nce_t, heads.contrast_weight, heads.reconstruct_weight,
            heads.partitions, heads.r1, heads.r2) == (0.1, 0.4, 0, 0, 8, 0.03, 8192, 0.4, 1, 1, 4, 0.125, 2)
    # v1m1 keeps its keys and has none of the CSC attributes
    plain = msc.MaskedSceneContrast(backbone=torch.nn.Linear(3, 4), backbone_in_channels=3, backbone_out_channels=4)
    assert not hasattr(plain, "partitions") and not hasattr(plain, "r1")
    # both transform lists build, fused and not
    g = torch.Generator().manual_seed(1)
    assert recorded["view1_transform"] == recorded["view2_transform"] and len(recorded["view1_transform"]) == 13
    for cfg in (recorded["view1_transform"], recorded["view2_transform"]):
        for fuse in (False, True):
            pipe = T.Compose(cfg, fuse=fuse, generator=g)
            assert [type(t).__name__ for t in pipe.transforms] == [c["type"] for c in cfg]


def test_pair_views_key_set():
    """ScanNetPairDataset.prepare_train_data: either frame through its own list, the results under view1_* and view2_*.  On the
    host with the entries of the recorded lists that are plain torch (Copy, NormalizeColor, ToTensor, Collect); the whole lists
    run on the GPU in tests/test_gpu_msc_csc_model.py"""
    from ao_amd.ptv2 import transform as T

    recorded = config()
    keep = ("Copy", "NormalizeColor", "ToTensor", "Collect")
    lists = [[c for c in recorded[k] if c["type"] in keep] for k in ("view1_transform", "view2_transform")]
    assert [c["type"] for c in lists[0]] == list(keep)
    g = torch.Generator().manual_seed(2)
    frames = [dict(coord=torch.rand(n, 3, generator=g), color=torch.rand(n, 3, generator=g) * 255,
                   discrete_coord=torch.randint(0, 40, (n, 3), generator=g)) for n in (50, 40)]
    out = T.pair_views(frames[0], frames[1], T.Compose(lists[0]), T.Compose(lists[1]))
    assert sorted(out) == sorted("view%d_%s" % (v, k) for v in (1, 2) for k in ("origin_coord", "discrete_coord", "coord", "color",
                                                                                 "offset", "feat"))
    assert out["view1_feat"].shape == (50, 3) and out["view2_feat"].shape == (40, 3) and out["view2_offset"].tolist() == [40]
    assert torch.equal(out["view1_origin_coord"], out["view1_coord"]) and float(out["view1_color"].max()) <= 1.0
    batch = T.point_collate([out, T.pair_views(frames[1], frames[0], T.Compose(lists[0]), T.Compose(lists[1]))])
    assert batch["view1_offset"].tolist() == [50, 90] and batch["view2_offset"].tolist() == [40, 90]


def test_op_refuses_the_host():
    from ao_amd import msc

    one = torch.tensor([4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        msc.csc_nce(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(4, 3), one,
                    torch.zeros((2, 2), dtype=torch.int64), 0.4, 0.125, 0.5)
