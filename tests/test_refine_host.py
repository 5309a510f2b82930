"""CPU: the host side of REAL's epoch-end label refinement (ao_amd/ptv2/refine.py, include/ptv2_refine_hip.h).

1. tests/refine_ref.py, the numpy restatement the GPU tests use for shapes the fixture does not hold, reproduces
   tests/golden/refine.npz (made by the reference's own statements) exactly: pred, conf (same fp32 arithmetic), the prompts
   in order, which prompts each view sees, the votes, the labels and the count.
2. `grid_cells` holds the reference's two differently parenthesised formulas.
3. The third header parses into tables of its own; every symbol is exported and bound; the version call answers 1.
4. The launchers refuse bad sizes before anything is enqueued (no GPU needed), and the ops refuse CPU tensors.
"""
import numpy as np
import pytest
import torch

from tests import refine_cases as RC
from tests import refine_ref as RR


@pytest.fixture(scope="module")
def fx():
    return RC.load()


@pytest.mark.parametrize("tag", sorted(RC.CASES))
def test_restatement_reproduces_the_reference(fx, tag):
    case = RC.room(tag)
    out = RR.refine_scene(case["logits"], case["coord"], case["label"], case["present"],
                          [(b, v) for v, b in enumerate(case["bridges"])], lambda v, uv, k: RC.masks_for(case, v, uv, k))
    assert np.array_equal(out["pred"], fx[tag + "_pred"]) and (out["pred"] == -1).sum() == RC.blocks(case["n"])[0].size > 0
    assert np.array_equal(out["conf"], fx[tag + "_conf"])
    assert np.array_equal(out["prompt_idx"], fx[tag + "_prompt_idx"]) and np.array_equal(out["prompt_cls"], fx[tag + "_prompt_cls"])
    assert out["seen"].tolist() == fx[tag + "_seen"].tolist() and out["seen"][-1] == 0
    assert np.array_equal(out["vote"], fx[tag + "_vote"])
    assert np.array_equal(out["label"], fx[tag + "_label"])
    assert out["updated"] == int(fx[tag + "_updated"]) > 0 and out["touched"] == bool(fx[tag + "_touched"]) is True
    # the float64 margin is within the recorded spread of the reference's fp32 one
    conf64 = RR.confidence(case["logits"], np.float64)[1]
    assert np.abs(out["conf"] - conf64).max() == float(fx[tag + "_conf_spread"]) < 1e-6


def test_the_fixture_inputs_meet_their_conditions():
    for tag in RC.CASES:
        case = RC.room(tag)
        rows, _ = RC.rivals(case["coord"], case["logits"], case["label"], case["present"])
        assert rows.size == 0, tag
        assert np.array_equal(case["logits"] * 4, np.round(case["logits"] * 4))
        _, src, higher, lower = RC.blocks(case["n"])
        assert src.size >= 30 and lower.max() < src.min() and src.max() < higher.min()
        assert np.array_equal(case["logits"][src], case["logits"][higher]) and np.array_equal(case["logits"][src], case["logits"][lower])


def test_grid_cells():
    from ao_amd.ptv2 import grid_cells

    assert grid_cells(0.0, 3.2, 0.0, 2.7, 0.5) == (8, 5)      # int(ceil(3.2) // 0.5), int(ceil(2.7 // 0.5))
    assert grid_cells(1.0, 4.2, -1.0, 1.7, 0.5) == (8, 5)
    assert grid_cells(0.0, 3.2, 0.0, 0.4, 0.5) == (8, 0)      # below one cell in y: no cell at all
    assert grid_cells(0.0, 0.3, 0.0, 0.6, 0.5) == (2, 1)      # x: a length below one cell still gives two
    assert grid_cells(0.0, 0.0, 0.0, 3.0, 0.5) == (0, 6)
    assert grid_cells(0.0, 3.0, 0.0, 3.0, 0.5) == (6, 6)
    for args in ((0.0, 3.2, 0.0, 2.7, 0.5), (1.0, 7.3, 0.0, 4.6, 0.5), (0.0, 0.3, 0.0, 0.4, 0.5)):
        assert grid_cells(*args) == RR.grid_cells(*args)
    with pytest.raises(ValueError):
        grid_cells(0.0, float("nan"), 0.0, 1.0)


def test_third_header_and_abi_version():
    from ao_amd import _abi, _lib

    names = ["ptv2_refine_abi_version", "refine_confidence_hip_launcher", "refine_prompts_hip_launcher",
             "refine_update_hip_launcher", "refine_vote_hip_launcher", "refine_workspace_bytes"]
    assert sorted(_abi.refine_signatures) == names
    assert not set(names) & (set(_abi.signatures) | set(_abi.data_signatures))
    assert not set(_abi.refine_consts) & (set(_abi.consts) | set(_abi.data_consts)) and _abi.refine_structs == {}
    assert _abi.refine_consts["PTV2_REFINE_MIN_C"] == 2 and _abi.refine_consts["PTV2_REFINE_MAX_C"] == 32
    assert [_abi.refine_consts["PTV2_REFINE_STATUS_" + n] for n in ("ERROR", "PROMPTS", "UPDATED")] == [0, 1, 2]
    L = _lib.lib()
    assert L.ptv2_refine_abi_version() == _lib.EXPECTED_REFINE_ABI == 1
    for name, (res, args) in _abi.refine_signatures.items():
        assert getattr(L, name).restype is res and getattr(L, name).argtypes == args, name
    assert [len(_abi.refine_signatures[n][1]) for n in names] == [0, 6, 20, 7, 16, 4]


def test_launchers_refuse_bad_sizes_before_enqueueing():
    from ao_amd import _abi, _lib

    L, ERR_ARG = _lib.lib(), _abi.consts["PTV2_ERR_ARG"]
    for n, c in ((10, 1), (10, 33), (-1, 13), (2 ** 31, 13)):
        assert L.refine_confidence_hip_launcher(n, c, 0, 0, 0, 0) == ERR_ARG
        assert L.refine_prompts_hip_launcher(n, c, 0, 0, 0, 0, 0, 0.0, 0.0, 2, 2, 0.5, 0.9, 0, 0, 0, 0, 0, 0, 0) == ERR_ARG
        assert L.refine_vote_hip_launcher(n, c, 0, 0, 0, 1, 0, 0, 4, 4, 0.9, 0, 0, 0, 0, 0) == ERR_ARG
        assert L.refine_update_hip_launcher(n, c, 0, 0, 0, 0, 0) == ERR_ARG
        assert L.refine_workspace_bytes(n, c, 4, 1) == -1
    # a NULL where one is not allowed, a grid that is not positive, an image without pixels
    assert L.refine_confidence_hip_launcher(10, 13, 0, 0, 0, 0) == ERR_ARG
    assert L.refine_update_hip_launcher(10, 13, 0, 0, 0, 0, 0) == ERR_ARG
    assert L.refine_prompts_hip_launcher(10, 13, 0, 0, 0, 0, 0, 0.0, 0.0, 2, 2, 0.0, 0.9, 0, 0, 0, 0, 0, 0, 0) == ERR_ARG
    assert L.refine_vote_hip_launcher(10, 13, 0, 0, 0, 1, 0, 0, 0, 4, 0.9, 0, 0, 0, 0, 0) == ERR_ARG
    # the workspace holds the table of the prompts (8 bytes per cell and class) or a view's scratch, whichever is larger
    assert L.refine_workspace_bytes(0, 13, 100, 0) >= 100 * 13 * 8
    assert L.refine_workspace_bytes(1000, 13, 0, 5) >= 1000 * 4 + 5 * 13 * 4 + 5 * 4


def test_no_cpu_fallback():
    from ao_amd import ptv2

    n, c = 8, 13
    logits, coord = torch.zeros(n, c), torch.zeros(n, 3)
    pred, conf, label = torch.zeros(n, dtype=torch.int32), torch.zeros(n), torch.zeros(n, dtype=torch.int32)
    present = torch.ones(c, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.scene_confidence(logits)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.grid_prompts(coord, pred, conf, label, present)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv2.LabelRefiner(c).begin(logits, coord, label, present)
    with pytest.raises(ValueError):
        ptv2.LabelRefiner(33)
