"""CPU: the host side of the instance evaluator (ao_amd/pointgroup/evaluate.py, include/ptv2_inseval_hip.h; DESIGN.md section
15): the numpy restatement of the association and `evaluate_matches` against the reference's recorded run, the header's
binding, the launcher's refusals, the rank order of `merge` and the registry."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import inseval_cases as C
from tests import inseval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "inseval.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def scenes():
    return C.scenes()


def recorded(fix, name):
    return {key: fix["%s.record.%s" % (name, key)] for key in C.RECORD_KEYS}


def assert_record(got, want, what):
    """every array of the record: dtype, shape and every element"""
    got = got._asdict() if hasattr(got, "_asdict") else got
    assert tuple(got) == C.RECORD_KEYS
    for key in C.RECORD_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].dtype, got[key].shape)
        assert np.array_equal(got[key], want[key]), (what, key)


def test_fixture_holds_the_cases(fixture, scenes):
    assert os.path.getsize(os.path.join(GOLDEN, "inseval.npz")) < 200 * 1024
    assert tuple(scenes) == C.SCENES
    for name, scene in scenes.items():
        assert scene["masks"].shape[1] == C.N and scene["masks"].dtype == np.int32
        for key, value in scene.items():
            stored = fixture["%s.%s" % (name, key)]
            if key == "masks":
                assert stored.dtype == np.uint8
                stored = stored.view(np.int8).astype(np.int32)
            assert stored.dtype == value.dtype and np.array_equal(stored, value), (name, key)
    assert np.array_equal(fixture["overlaps"], np.append(np.arange(0.5, 0.95, 0.05), 0.25))
    # what the scenes were written for, in the reference's own output
    a, b = recorded(fixture, "a"), recorded(fixture, "b")
    assert a["pred_row"].tolist() == [0, 1, 2, 3, 4, 7, 8, 9, 10, 11], "the small proposal and the ignored class are dropped"
    assert a["gt_instance_id"].tolist() == [3, 7, 12, 21, 40, 90] and a["gt_vert_count"][4] == 60
    assert a["pred_void"][3] == 100 and a["inter"][4, 4] == 60
    assert a["inter"][9, 1] == 0 and a["inter"][7, 1] == 0 and (a["inter"][2, 1:3] == 100).all()
    assert a["pred_conf"][0] == np.float64(np.float32(0.9)) != 0.9
    assert b["gt_instance_id"].tolist() == [2, 5, 6, 100] and b["pred_conf"][0] == a["pred_conf"][6] == 0.75
    table = fixture["ap_table"]
    assert table.shape == (6, 10) and np.isnan(table[[2, 4]]).all() and (table[[3, 5]] == 0).all()
    assert np.isfinite(table[:2]).all() and (table[:2] > 0).all() and len(np.unique(table[:2])) >= 6


@pytest.mark.parametrize("name", C.SCENES)
def test_ref_reproduces_the_recorded_records(fixture, scenes, name):
    s = scenes[name]
    got = R.associate(s["masks"], s["scores"], s["classes"], s["segment"], s["instance"], C.SEGMENT_IGNORE, C.INSTANCE_IGNORE,
                      C.MIN_REGION)
    assert_record(got, recorded(fixture, name), name)


def test_evaluate_matches_reproduces_the_recorded_table(fixture):
    """float64 sums of at most a few hundred terms in [0, 1]: only the order of np.dot's sum can differ, about 1e-14"""
    from ao_amd.pointgroup.evaluate import SceneMatches, evaluate_matches

    records = [SceneMatches(**recorded(fixture, name)) for name in C.SCENES]
    valid = fixture["valid_class_ids"].tolist()
    assert valid == [1, 2, 3, 4, 5, 6]
    names = [C.NAMES[i] for i in valid]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (nanmean over the all-NaN classes, as in the reference)
        got = evaluate_matches(records, valid, names)
    table, want = got["ap_table"], fixture["ap_table"]
    assert table.shape == want.shape == (6, 10) and np.array_equal(np.isnan(table), np.isnan(want))
    finite = np.isfinite(want)
    print("ap_table: max |difference| %.3g" % np.abs(table[finite] - want[finite]).max())
    assert np.abs(table[finite] - want[finite]).max() <= 1e-12
    for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert abs(float(got[key]) - float(fixture["ap_scores." + key])) <= 1e-12, key
    for key in ("ap", "ap50%", "ap25%"):
        have = np.array([got["classes"][n][key] for n in names])
        want_k = fixture["ap_scores.classes." + key]
        assert np.array_equal(np.isnan(have), np.isnan(want_k)), key
        assert np.abs(have[np.isfinite(want_k)] - want_k[np.isfinite(want_k)]).max() <= 1e-12, key
    assert list(got["classes"]) == names
    # one overlap at a time gives the same columns (the greedy state is reset per overlap), and the scene order matters to
    # nothing but the ties, which the thresholds absorb
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        one = evaluate_matches(records[::-1], valid, names, overlaps=[fixture["overlaps"][4], 0.25])
    assert np.abs(one["ap_table"][finite[:, [4, 9]]] - want[:, [4, 9]][finite[:, [4, 9]]]).max() <= 1e-12


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    assert set(_abi.inseval_signatures) == {"ptv2_inseval_abi_version", "inseval_associate_hip_launcher"}
    assert not _abi.inseval_structs
    with open(_abi.INSEVAL_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.inseval_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_inseval_abi_version() == _lib.EXPECTED_INSEVAL_ABI == 1
    consts = _abi.inseval_consts
    assert consts["INSEVAL_MAX_PROPOSALS"] == 65535 and consts["INSEVAL_BINS"] >= 64
    assert consts["INSEVAL_POINTS_PER_WG"] % 256 == 0
    # the other headers are as they were
    assert _lib.EXPECTED_ABI == 11 and L.ptv2_abi_version() == 11 and L.ptv2_pg_abi_version() == 1
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert "ptv2_inseval_hip.h" in f.read(), "the build digest covers the header"


def test_launcher_refuses_before_it_enqueues():
    """PTV2_ERR_ARG without a GPU: the checks come before the first runtime call (the pointers are never read)"""
    from ao_amd import _abi, _lib

    L = _lib.lib()
    err = _abi.consts["PTV2_ERR_ARG"]
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    call = L.inseval_associate_hip_launcher
    assert call(65536, 8, 8, 1, p, None, p, p, p, p, None) == err, "P > 65535"
    assert call(2, 8, -1, 1, p, p, p, p, p, p, None) == err, "negative n"
    assert call(2, -8, 8, 1, p, p, p, p, p, p, None) == err and call(-1, 8, 8, 1, p, None, p, p, p, p, None) == err
    assert call(2, 8, 8, 1, None, None, p, p, p, p, None) == err, "NULL masks"
    assert call(2, 8, 8, 1, p, None, None, p, p, p, None) == err and call(2, 8, 8, 1, p, None, p, None, p, p, None) == err
    assert call(2, 8, 8, 1, p, None, p, p, None, p, None) == err and call(2, 8, 8, 1, p, None, p, p, p, None, None) == err
    assert call(2, 8, 9, 1, p, None, p, p, p, p, None) == err, "no nn_idx: n == m"
    assert call(2, 8, 8, _abi.inseval_consts["INSEVAL_BINS"] + 1, p, None, p, p, p, p, None) == err, "one window per call"
    assert call(0, 8, 8, 1, None, None, None, None, None, None, None) == _abi.consts["PTV2_OK"], "no proposal: nothing to do"


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_no_cpu_fallback(path, monkeypatch, scenes):
    from ao_amd.pointgroup import associate

    monkeypatch.setenv("AO_AMD_INSEVAL", path)
    s = scenes["a"]
    pred = dict(pred_masks=torch.from_numpy(s["masks"]), pred_scores=torch.from_numpy(s["scores"]),
                pred_classes=torch.from_numpy(s["classes"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        associate(pred, torch.from_numpy(s["segment"]), torch.from_numpy(s["instance"]), C.NUM_CLASSES, C.SEGMENT_IGNORE)


def test_constructor_and_merge():
    from ao_amd.pointgroup import InsSegEvaluator

    ev = InsSegEvaluator()
    assert ev.segment_ignore_index == (-1,) and ev.instance_ignore_index == -1 and ev.min_region_sizes == 100
    assert np.array_equal(ev.overlaps, np.append(np.arange(0.5, 0.95, 0.05), 0.25))
    assert ev.distance_threshes == float("inf") and ev.distance_confs == -float("inf") and ev.valid_class_names is None
    ev = InsSegEvaluator(segment_ignore_index=(-1, 0, 1), instance_ignore_index=-2)
    assert ev.segment_ignore_index == (-1, 0, 1) and ev.instance_ignore_index == -2
    assert ev.merge([["r0s0", "r0s1"], [], ["r2s0"], ["r3s0", "r3s1"]]) == ["r0s0", "r0s1", "r2s0", "r3s0", "r3s1"], "rank order"


def test_registry_files_the_hook():
    from ao_amd.pointgroup import InsSegEvaluator
    from ao_amd.ptv2 import registry

    class Fake:
        def __init__(self):
            self.modules = {}

        def register_module(self, module=None, name=None, force=False):
            self.modules[name] = module

    models, hooks = Fake(), Fake()
    before = registry.register(MODELS=Fake())
    done = registry.register(MODELS=models, HOOKS=hooks)
    assert done == before == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image"], "filed and not listed"
    assert hooks.modules == {"InsSegEvaluator": InsSegEvaluator}
    assert registry.register(HOOKS=Fake()) == []
