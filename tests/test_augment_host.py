"""CPU: the training augmentations' host side (ao_amd/ptv2/transform.py) and their numpy restatement (tests/augment_ref.py).

1. `build_transform` accepts every active `type=` of the reference's semseg-pt-v2m2-* / semseg-cac-v1m1-2-ptv2-* train and
   validation lists (tests/golden/augment_train_types.json: names and arguments as data).
2. The Philox4x32-10 restatement gives the Random123 known answers.
3. The programs `Compose(fuse=True)` plans for the two train prefixes -- step kinds, flags, round-step placement, segment
   cuts -- equal the expectations written out below.
4. The numpy interpreter, run on the planned programs with the recorded draws, reproduces the fixture
   (tests/golden/augment.npz, made by the reference's own transform.py): colour bit-equal, coord bit-equal where no rotation
   precedes; after a rotation within 1 fp32 ulp with at most 0.1 % of the entries differing (the reference's BLAS np.dot may
   fuse).  Measured for the fixture's 303-point cloud: 0 differing entries in every case, rotations included.
5. The Mix3D collate gives the reference's offsets for 2, 3 and 4 scenes.
6. The second header parses into tables of its own and both ABI-version calls answer.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import augment_cases as C
from tests import augment_ref as R
from tests.conftest import GOLDEN

K = None


@pytest.fixture(scope="module")
def T():
    from ao_amd.ptv2 import transform

    return transform


@pytest.fixture(scope="module")
def fx():
    return C.load()


def test_build_transform_accepts_the_train_lists(T):
    with open(os.path.join(GOLDEN, "augment_train_types.json")) as f:
        cfgs = json.load(f)
    assert {c["type"] for c in cfgs} >= {"RandomRotate", "RandomJitter", "ElasticDistortion", "ChromaticAutoContrast",
                                         "ChromaticTranslation", "ChromaticJitter", "ShufflePoint", "PointClip", "Copy"}
    for cfg in cfgs:
        assert type(T.build_transform(cfg)).__name__ == cfg["type"]
    for name in ("RandomShift", "RandomColorDrop"):
        assert type(T.build_transform(dict(type=name))).__name__ == name
    T.Compose(cfgs, fuse=True)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    out = R.philox4x32_10(np.array([counter], np.uint64), key)
    assert tuple(int(v) for v in out[0]) == want


def test_normals_are_standard(T):
    g = R.normals64(200000, seed=12345, stream=3)
    assert np.abs(g).max() <= np.sqrt(2 * 25 * np.log(2))  # the smallest uniform is 2^-25
    for col in g.T:
        assert abs(col.mean()) < 5 / np.sqrt(g.shape[0]) and abs(col.var() - 1) < 5 * np.sqrt(2 / g.shape[0])
    assert not np.array_equal(g, R.normals64(200000, seed=12345, stream=4))
    assert np.array_equal(g[100:165], R.normals64(65, seed=12345, stream=3, first=100))


def plan_of(T, fx, tag):
    cfg, draws = C.case(fx, tag)
    comp = T.Compose(cfg, fuse=True)
    plans = comp.plan(dict(seed=0, per=draws))
    assert len(plans) == 1
    return plans[0]


def shape_of(segs):
    return [(s["bounds"], s["readback"], s["out_f64"], [(st["kind"], st["flags"]) for st in s["steps"]]) for s in segs]


def test_planned_programs_of_the_train_prefixes(T, fx):
    k = T._K
    CS, ROT, SC, J, EL, RND = (k["PTV2_AUG_" + n] for n in ("CENTER_SHIFT", "ROTATE", "SCALE", "JITTER", "ELASTIC", "ROUND_F32"))
    CC, CT, CJ = (k["PTV2_AUG_COLOR_" + n] for n in ("CONTRAST", "TRANSLATE", "JITTER"))
    F32, Z, BC = k["PTV2_AUG_FLAG_FP32"], k["PTV2_AUG_FLAG_APPLY_Z"], k["PTV2_AUG_FLAG_BOUNDS_CENTER"]
    r = (RND, 0)
    # S3DIS: everything is float32, so every coordinate step is followed by a round; the colour bounds of the one bounds
    # launch are still current at the auto-contrast: ONE segment
    assert shape_of(plan_of(T, fx, "s3dis_prefix")) == [
        (True, False, False, [(CS, F32 | Z), r, (SC, F32), r, (SC, F32), r, (J, F32), r, (CC, 0), (CT, 0), (CJ, 0)])]
    # ScanNet: float32 up to the z rotation (which still rounds its centred coordinate), float64 after it; the x and y
    # rotations about the box centre and each elastic pair read bounds of the current state: five cuts; the final round
    assert shape_of(plan_of(T, fx, "scannet_prefix")) == [
        (True, False, True, [(CS, F32 | Z), r, (ROT, F32)]),
        (True, False, True, [(ROT, BC)]),
        (True, False, True, [(ROT, BC), (SC, 0), (SC, 0), (J, 0)]),
        (True, True, True, [(EL, 0)]),
        (True, True, False, [(EL, 0), (CC, 0), (CT, 0), (CJ, 0), r])]
    # stream numbers: 8 per transform of the list, the elastic pairs at +1, +2
    streams = [st.get("stream") for s in plan_of(T, fx, "scannet_prefix") for st in s["steps"] if st["kind"] in (J, EL, CJ)]
    assert streams == [48, 57, 58, 80]


def test_a_long_list_is_cut_at_the_step_limit(T):
    recs = [dict(kind=T._K["PTV2_AUG_SHIFT"], p=[0.0, 0.0, 0.0]) for _ in range(20)]
    segs = T.fuse_plan(recs, final_round=True)
    assert all(len(s["steps"]) <= T._K["PTV2_AUG_MAX_STEPS"] for s in segs) and len(segs) == 3
    assert sum(st["kind"] == T._K["PTV2_AUG_SHIFT"] for s in segs for st in s["steps"]) == 20
    assert [s["out_f64"] for s in segs] == [True, True, False]


def cases(fx):
    return json.loads(str(fx["cases"]))


def test_interpreter_reproduces_the_reference(T, fx):
    assert len(cases(fx)) == 22
    for tag in cases(fx):
        cfg, draws = C.case(fx, tag)
        comp = T.Compose(cfg, fuse=True)
        recs = comp.records(range(len(cfg)), dict(seed=0, per=draws))
        elastic = any(c["type"] == "ElasticDistortion" and d["gate"] < 0.95 for c, d in zip(cfg, draws))
        for final_round in (False, True):
            segs = T.fuse_plan(recs, in_f64=False, final_round=final_round)
            if not segs:
                assert tag.endswith("_off")
                coord, color = fx["coord"], fx["color"]
            else:
                coord, color = R.run_plan(segs, fx["coord"], fx["color"], elastic_grid=T.elastic_grid)
            if not final_round:  # a class on its own returns the reference's dtype
                assert coord.dtype == fx[tag + "_coord"].dtype, tag
            else:
                assert coord.dtype == np.float32
            assert C.check_against_fixture(fx, tag, coord, color, elastic) == 0, tag  # (measured: none differ)


def test_blur_restatement_equals_scipy(fx):
    grid = fx["blur_in"]
    assert grid.shape == (10, 8, 6, 3)
    for i in range(6):
        grid = R.blur3(grid, i % 3)
        assert np.array_equal(grid, fx["blur_pass%d" % i]), i


@pytest.mark.parametrize("scenes", [2, 3, 4])
def test_mix3d_collate(T, scenes):
    sizes = [5, 3, 4, 6][:scenes]
    batch = [dict(coord=torch.zeros(n, 3), offset=torch.tensor([n])) for n in sizes]
    plain = T.point_collate([dict(b) for b in batch])
    ends = np.cumsum(sizes).tolist()
    assert plain["offset"].tolist() == ends and plain["offset_host"] == ends
    mixed = T.point_collate([dict(b) for b in batch], mix=True)
    want = torch.cat([torch.tensor(ends)[1:-1:2], torch.tensor(ends)[-1:]]).tolist()  # datasets/utils.py:51-53
    assert mixed["offset"].tolist() == want and mixed["offset_host"] == want and mixed["coord"].shape[0] == ends[-1]
    assert want == {2: [8], 3: [8, 12], 4: [8, 18]}[scenes]
    g = torch.Generator().manual_seed(0)
    assert T.point_collate([dict(b) for b in batch], mix_prob=0, generator=g)["offset"].tolist() == ends
    assert T.point_collate([dict(b) for b in batch], mix_prob=1, generator=g)["offset"].tolist() == want


def test_second_header_and_abi_versions():
    from ao_amd import _abi, _lib

    assert len(_abi.signatures) == 127 and not set(_abi.signatures) & set(_abi.data_signatures)
    assert sorted(_abi.data_signatures) == ["aug_blur3_hip_launcher", "aug_bounds_hip_launcher", "aug_noise_hip_launcher",
                                            "aug_points_hip_launcher", "ptv2_data_abi_version", "ptv2_data_struct_bytes"]
    assert list(_abi.data_structs) == ["ptv2_aug_step", "ptv2_aug_program"] and "ptv2_aug_step" not in _abi.structs
    assert _abi.data_consts["PTV2_AUG_MAX_STEPS"] == 16 and "PTV2_AUG_MAX_STEPS" not in _abi.consts
    # the whole program travels as one kernel argument: it has to stay under the 4 KiB of a kernarg segment
    assert ctypes.sizeof(_abi.data_structs["ptv2_aug_program"]) == 2192
    L = _lib.lib()
    assert _lib._SIGNATURES is _abi.signatures
    assert L.ptv2_abi_version() == _lib.EXPECTED_ABI == 11 and L.ptv2_data_abi_version() == _lib.EXPECTED_DATA_ABI == 1
    for name, (res, args) in _abi.data_signatures.items():
        assert getattr(L, name).restype is res and getattr(L, name).argtypes == args, name
    assert L.ptv2_data_struct_bytes(1) == 2192 and L.ptv2_data_struct_bytes(0) == 136
