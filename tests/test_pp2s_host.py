"""CPU: the host side of the PP2S label pipeline (ao_amd/ptv2/pp2s.py, include/ptv2_pp2s_hip.h).

1. tests/pp2s_ref.py, the numpy restatement the GPU tests use for shapes the fixture does not hold, reproduces
   tests/golden/pp2s.npz (made by the reference's own statements) exactly: the bridges, the visible count of every view,
   seen_any, the weak mask, the prompts each view sees, the labels; the aligned room within the derived bound.
2. The fixture's inputs meet the conditions under which the reference alone is unambiguous, and hold the cases they promise.
3. The fourth header parses into tables of its own; every symbol is exported and bound; the version call answers 1.
4. The launchers refuse bad sizes before anything is enqueued (no GPU needed), and the ops refuse CPU tensors.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import pp2s_cases as PC
from tests import pp2s_ref as PR


@pytest.fixture(scope="module")
def fx():
    return PC.load()


@pytest.mark.parametrize("tag", sorted(PC.CASES))
def test_restatement_reproduces_the_reference(fx, tag):
    case = PC.room(tag)
    want = PC.expected(fx, case)
    out = PR.pp2s_scene(case["coord"], case["instance"], case["semantic"], PC.view_args(case),
                        lambda key, xy, cls: PC.masks_for(case, key, xy, cls), case["c"], case["angle"], case["center"])
    err = np.abs(out["coord64"][::PC.ALIGN_STRIDE] - want["aligned"])
    print("aligned: max |restatement - fixture| = %.3e" % err.max())
    assert (err <= PC.align_bound(case, slice(None, None, PC.ALIGN_STRIDE))).all()
    empty = (np.zeros(0, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.int32))
    for v, view in enumerate(case["views"]):
        assert out["visible"][view["key"]] == want["visible"][v]
        got = out["bridges"].get(view["key"])
        assert (got is None) == (want["visible"][v] == 0)
        assert np.array_equal(got if got is not None else np.zeros((case["n"], 3), np.int32), want["bridges"][v])
        idx, xy, cls = out["prompts"].get(view["key"], empty)  # (no bridge file: not a frame)
        assert np.array_equal(idx, want["prompts"][v][0]) and np.array_equal(xy, want["prompts"][v][1])
        assert np.array_equal(cls, want["prompts"][v][2])
    assert np.array_equal(out["seen_any"], want["seen_any"]) and np.array_equal(out["weak"], want["weak"])
    assert out["label"].shape == (case["n"], 1) and np.array_equal(out["label"][:, 0], want["label"])
    # the last view sees nothing, the one before it points but no weak point
    assert want["visible"][-1] == 0 and want["visible"][case["quiet"]] > 0 and want["prompts"][case["quiet"]][0].size == 0


def test_the_fixture_inputs_meet_their_conditions(fx):
    for tag in PC.CASES:
        case = PC.room(tag)
        want = PC.expected(fx, case)
        coord64 = PR.align(case["coord"], case["angle"], case["center"])
        k = case["views"][0]["k"]
        assert k[0, 2] != k[1, 2] and case["views"][0]["depth"].shape == (case["size"][1], case["size"][0])
        for view in case["views"]:
            m = PR.project(coord64, view["k"], view["rt"], view["depth"] / PC.DEPTH_SCALE, PC.TOL, margins=True)[3]
            assert min(m.values()) > 1e-6, (tag, view["key"], m)
        inst, sem = case["instance"].reshape(-1), case["semantic"].reshape(-1)
        ids, counts = np.unique(inst, return_counts=True)
        seen_per = np.array([want["seen_any"][inst == i].sum() for i in ids])
        assert 12 <= ids.size <= 30 and -1 in ids and (counts == 1).any() and (seen_per == 2).any() and (seen_per == 0).any()
        assert want["weak"].sum() == ids.size and (sem[want["weak"] == 1] == -1).any()
        assert ((want["label"] == -1) & (want["seen_any"] == 1)).any() and (want["label"][want["weak"] == 0] != -1).sum() > 100


def test_the_emulated_fused_multiply_add_is_exact():
    rng = np.random.default_rng(3)
    a, b, c = rng.standard_normal(400) * 5, rng.standard_normal(400), rng.standard_normal(400) * 3
    c[:50] = -(a[:50] * b[:50])  # cancellation: the product's rounding error is all that is left
    want = [float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)]
    assert np.array_equal(PR.fma(a, b, c), np.array(want))
    from ao_amd.ptv2 import pp2s

    assert np.array_equal(pp2s._fma(torch.tensor(a), torch.tensor(b), torch.tensor(c)).numpy(), np.array(want))
    assert pp2s.rotation(33) == tuple(float(v) for v in PR.rotation(33))


def test_weak_choice_restated():
    inst = np.array([7, 7, 7, 7, 7, -1, -1, -1, 9, 9, 2 ** 31 - 1, -2 ** 31, -2 ** 31], np.int32)
    seen = np.array([0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    # 7: seen 1, 3, 4 -> rank 1 = 3;  -1: unseen, 3 points -> rank 1 = 6;  9: seen 8, 9 -> rank 1 = 9;  the single point;
    # INT_MIN: one seen -> rank 0 = 11
    assert np.nonzero(PR.weak_mask(inst, seen))[0].tolist() == [3, 6, 9, 10, 11]


def test_fourth_header_and_abi_version():
    from ao_amd import _abi, _lib

    names = ["pp2s_align_hip_launcher", "pp2s_labels_hip_launcher", "pp2s_pixel_labels_hip_launcher", "pp2s_project_hip_launcher",
             "pp2s_vote_hip_launcher", "pp2s_weak_hip_launcher", "pp2s_workspace_bytes", "ptv2_pp2s_abi_version"]
    assert sorted(_abi.pp2s_signatures) == names
    others = (set(_abi.signatures) | set(_abi.data_signatures) | set(_abi.refine_signatures))
    assert not set(names) & others
    assert not set(_abi.pp2s_consts) & (set(_abi.consts) | set(_abi.data_consts) | set(_abi.refine_consts)) and _abi.pp2s_structs == {}
    assert _abi.pp2s_consts["PTV2_PP2S_MIN_C"] == 2 and _abi.pp2s_consts["PTV2_PP2S_MAX_C"] == 32
    assert _abi.pp2s_consts["PTV2_PP2S_MAX_BOUND"] == 65535
    assert [_abi.pp2s_consts["PTV2_PP2S_STATUS_" + n] for n in ("ERROR", "VISIBLE")] == [0, 1]
    assert [_abi.pp2s_consts["PTV2_PP2S_BAD_" + n] for n in ("PIXEL", "CLASS")] == [1, 2]
    L = _lib.lib()
    assert L.ptv2_pp2s_abi_version() == _lib.EXPECTED_PP2S_ABI == 1 and _lib.EXPECTED_ABI == 11
    for name, (res, args) in _abi.pp2s_signatures.items():
        assert getattr(L, name).restype is res and getattr(L, name).argtypes == args, name
    assert [len(_abi.pp2s_signatures[n][1]) for n in names] == [9, 6, 10, 36, 9, 7, 3, 0]


def test_launchers_refuse_bad_sizes_before_enqueueing():
    from ao_amd import _abi, _lib

    L, ERR_ARG = _lib.lib(), _abi.consts["PTV2_ERR_ARG"]
    mats = [0.0] * 24

    def project(n, depth_h=4, depth_w=4, height=3.0, width=3.0, tol=0.1, status=1):
        return L.pp2s_project_hip_launcher(n, 0, *mats, 0, depth_h, depth_w, height, width, tol, 0, 0, status, 0)

    for n in (-1, 2 ** 31):
        assert L.pp2s_align_hip_launcher(n, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 0, 0) == ERR_ARG
        assert project(n) == ERR_ARG
        assert L.pp2s_weak_hip_launcher(n, 0, 0, 0, 0, 0, 0) == ERR_ARG
        assert L.pp2s_vote_hip_launcher(n, 0, 4, 4, 0, 0, 0, 1, 0) == ERR_ARG
        assert L.pp2s_labels_hip_launcher(n, 0, 0, 0, 0, 0) == ERR_ARG
        assert L.pp2s_workspace_bytes(n, 4, 4) == -1
    # a NULL where one is not allowed (the non-zero "pointers" are never dereferenced: the call returns first)
    assert L.pp2s_align_hip_launcher(10, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 0, 0) == ERR_ARG
    assert project(10) == ERR_ARG and project(10, status=0) == ERR_ARG
    assert L.pp2s_weak_hip_launcher(10, 0, 0, 0, 0, 0, 0) == ERR_ARG
    assert L.pp2s_vote_hip_launcher(10, 0, 4, 4, 0, 0, 0, 1, 0) == ERR_ARG
    assert L.pp2s_labels_hip_launcher(10, 0, 0, 0, 0, 0) == ERR_ARG
    # a bound above uint16 (or a NaN), an image without pixels, a negative tolerance
    assert project(0, height=65536.0) == ERR_ARG and project(0, width=float("nan")) == ERR_ARG
    assert project(0, depth_h=0) == ERR_ARG and project(0, tol=-1.0) == ERR_ARG
    assert L.pp2s_vote_hip_launcher(10, 0, 0, 4, 0, 0, 0, 1, 0) == ERR_ARG
    # classes outside [2, 32], a negative prompt count, no workspace
    for prompts, c, ws in ((1, 1, 1), (1, 33, 1), (-1, 13, 1), (1, 13, 0)):
        assert L.pp2s_pixel_labels_hip_launcher(prompts, c, 0, 0, 4, 4, ws, 1024, 1, 0) == ERR_ARG
    assert L.pp2s_workspace_bytes(10, -1, 4) == -1 and L.pp2s_workspace_bytes(0, 65536, 65536) == -1
    # nothing to do: no launch, no error
    assert L.pp2s_align_hip_launcher(0, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 0, 0) == 0
    assert project(0) == 0 and L.pp2s_weak_hip_launcher(0, 0, 0, 0, 0, 0, 0) == 0
    assert L.pp2s_vote_hip_launcher(0, 0, 4, 4, 0, 0, 0, 1, 0) == 0 and L.pp2s_labels_hip_launcher(0, 0, 0, 0, 0, 0) == 0
    assert L.pp2s_workspace_bytes(0, 47, 63) >= 47 * 63 * 4


def test_no_cpu_fallback():
    from ao_amd import ptv2

    n = 8
    coord, inst = torch.zeros(n, 3), torch.zeros(n, dtype=torch.int32)
    seen, gt = torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32)
    k, rt = np.eye(3), np.eye(3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.align_room(coord, 90, (0.0, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.project_view(coord.double(), k, rt, torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.choose_weak_labels(inst, seen)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.LabelPropagator(gt, seen, 13)
