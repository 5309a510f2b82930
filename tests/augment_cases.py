"""Shared by tests/test_augment_host.py and tests/test_gpu_augment.py (no test in here): the fixture's cases as the classes
of ao_amd.ptv2.transform take them."""
import json
import os

import numpy as np

from tests.conftest import GOLDEN


def load():
    return np.load(os.path.join(GOLDEN, "augment.npz"))


def case(fx, tag, tensor=np.asarray):
    """(cfg list, draws list with the recorded arrays put in through `tensor`)"""
    def put(v):
        if isinstance(v, dict) and "npz" in v:
            return tensor(fx[v["npz"]])
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return [put(x) for x in v]
        return v

    cfg = json.loads(str(fx[tag + "_cfg"]))
    draws = [{k: put(v) for k, v in d.items()} for d in json.loads(str(fx[tag + "_draws"]))]
    return cfg, draws


def ulp32(x):
    """one fp32 unit in the last place at the magnitude of x"""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def check_against_fixture(fx, tag, coord, color, elastic):
    """the bounds of the issue: colour bit-equal; coord bit-equal where no rotation precedes, else within 1 fp32 ulp with at
    most 0.1 % of the entries differing; with an elastic step, within max(4 elastic_ref_err, 1 fp32 ulp).  Returns the
    number of differing coordinate entries."""
    want, want_color = fx[tag + "_coord"], fx[tag + "_color"]
    assert np.array_equal(np.asarray(color), want_color), tag
    cfg = json.loads(str(fx[tag + "_cfg"]))
    draws = json.loads(str(fx[tag + "_draws"]))
    rotated = any(c["type"] == "RandomRotate" and d["angle"] is not None for c, d in zip(cfg, draws))
    have = np.asarray(coord, np.float64)
    want32 = want.astype(np.float32).astype(np.float64)  # (the fused result is rounded to fp32 at its end, as ToTensor does)
    if np.asarray(coord).dtype == np.float32 or rotated:  # (after a rotation the bound is stated on fp32 values)
        have, want = have.astype(np.float32).astype(np.float64), want32
    diff = np.abs(have - want)
    if elastic:
        assert (diff <= np.maximum(4 * float(fx["elastic_ref_err"]), ulp32(want))).all(), (tag, diff.max())
    elif rotated:
        assert (diff <= ulp32(want)).all(), (tag, diff.max())
        assert (diff > 0).sum() <= 1e-3 * diff.size, (tag, int((diff > 0).sum()))
    else:
        assert (diff == 0).all(), (tag, diff.max())
    return int((diff > 0).sum())
