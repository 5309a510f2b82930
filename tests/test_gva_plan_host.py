"""CPU: gva_plan() (ao_amd/csrc/gva_plan.hip), the one place that picks the kernel form of every attention stage, through the
host-only ptv2_gva_plan_describe.

1. The plan of every grid case equals tests/golden/gva_plan.npz.  That table was recorded from the build of the commit
   before gva_plan() existed: a script loaded that libptv2_hip.so with ctypes, called its host-only predicates
   (gva_*_supported, gva_bwd_point_local, gva_block_keeps_A, gva_bwd_tile_path, gva_bwd_staged, gva_fwd_point_max_n) by their
   mangled names and composed the conditions that were then written inline in gva_block.hip, gva_aggregate.hip, gva_fwd.hip
   and gva_bwd.hip.  Columns of `cases`: env, n, k, c, g, attn_drop, has_inverse; of `plan`: the 12 ints of the header.
2. What sizing and running have to agree on: wp2_recompute == !keeps_A; the workspace has g_A / g_sw exactly when the plan is
   not fused_peb; the saved region has A exactly when the plan keeps it (so never for a tile forward that does not write it).
3. ao_amd.ptv2.gva.dropout_supported() says what the plan's bwd_takes_dropout says.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests.conftest import ROOT

SWITCHES = ("AO_AMD_FWD_STAGED", "AO_AMD_BWD_STAGED", "AO_AMD_BWD_POINT", "AO_AMD_TILE_KEEP_A")
ENVS = list(range(16)) + [16]  # bit i: SWITCHES[i] is set; 16: AO_AMD_LOGITS_BWD=staged alone
KS = (8, 16, 32)
SHAPES = ((6, 48), (12, 96), (24, 192), (48, 384), (64, 512), (6, 24), (8, 64))  # (g, c)
FWD_POINT_MAX_N = ((0x7FFFFFFF // (4 * 6 * 48)) & ~63) - 64  # gva_fwd_point_max_n() (gva_fwd_point.hip)
NS = (1, 1074, 120000, FWD_POINT_MAX_N + 64)
FIELDS = ("logits_fwd", "fwd", "softmax", "bwd_agg", "bwd_agg_given_gA", "logits_bwd", "keeps_A", "fused_peb", "wp2_recompute",
          "bwd_takes_dropout", "bwd_tile_shape", "g_slot")
F = {name: i for i, name in enumerate(FIELDS)}
F_POINT, F_TILE, F_STAGED = 0, 1, 2


def set_env(monkeypatch, env):
    for i, name in enumerate(SWITCHES):
        if env < 16 and env >> i & 1:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    if env == 16:
        monkeypatch.setenv("AO_AMD_LOGITS_BWD", "staged")
    else:
        monkeypatch.delenv("AO_AMD_LOGITS_BWD", raising=False)


def shape_cases():
    return itertools.product(KS, SHAPES, NS, (0, 1), (0, 1))


@pytest.fixture(scope="module")
def L():
    from ao_amd import _lib
    import ao_amd.ptv2.block  # noqa: F401  (ptv2_block_saved_bytes)
    import ao_amd.ptv2.gva  # noqa: F401  (gva_block_workspace_bytes)

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def describe(L, n, k, c, g, drop, inv):
    out = (ctypes.c_int * len(FIELDS))()
    assert L.ptv2_gva_plan_describe(n, k, c, g, drop, inv, out, len(FIELDS)) == 0
    return list(out)


def test_describe_rejects_bad_arguments(L):
    out = (ctypes.c_int * len(FIELDS))()
    assert L.ptv2_gva_plan_describe(100, 16, 48, 6, 0, 1, out, len(FIELDS) - 1) == 1  # PTV2_ERR_ARG
    assert L.ptv2_gva_plan_describe(100, 16, 48, 6, 0, 1, None, len(FIELDS)) == 1
    assert L.ptv2_gva_plan_describe(100, 0, 48, 6, 0, 1, out, len(FIELDS)) == 1


def test_plan_equals_the_recorded_table(L, monkeypatch):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gva_plan.npz"))
    cases, plan = gold["cases"], gold["plan"]
    assert plan.shape == (len(cases), len(FIELDS))
    want = {tuple(int(v) for v in row): [int(v) for v in p] for row, p in zip(cases, plan)}
    seen = 0
    for env in ENVS:
        set_env(monkeypatch, env)
        for k, (g, c), n, drop, inv in shape_cases():
            key = (env, n, k, c, g, drop, inv)
            got = describe(L, n, k, c, g, drop, inv)
            assert got == want[key], (key, dict(zip(FIELDS, got)), dict(zip(FIELDS, want[key])))
            seen += 1
    assert seen == len(want) == len(cases) == len(ENVS) * len(KS) * len(SHAPES) * len(NS) * 4
    # the table itself exercises every form
    for name, forms in (("logits_fwd", 3), ("fwd", 3), ("softmax", 2), ("bwd_agg", 4), ("logits_bwd", 3)):
        assert set(plan[:, F[name]].tolist()) == set(range(forms)), name
    # ... and the row bound of the full-resolution forward kernel
    set_env(monkeypatch, 0)
    assert describe(L, FWD_POINT_MAX_N, 16, 48, 6, 0, 1)[F["fwd"]] == F_POINT
    assert describe(L, FWD_POINT_MAX_N + 64, 16, 48, 6, 0, 1)[F["fwd"]] == F_STAGED


def al(v):
    return (v + 255) & ~255


def test_sizing_and_running_agree(L, monkeypatch):
    for k, (g, c), n in itertools.product(KS, SHAPES, NS):
        ws_rest, saved_rest = set(), set()
        for env in ENVS:
            set_env(monkeypatch, env)
            ws, saved = L.gva_block_workspace_bytes(n, k, c, g), L.ptv2_block_saved_bytes(n, k, c, g)
            for drop, inv in itertools.product((0, 1), (0, 1)):
                p = dict(zip(FIELDS, describe(L, n, k, c, g, drop, inv)))
                case = (env, n, k, c, g, drop, inv)
                assert p["wp2_recompute"] == (not p["keeps_A"]), case
                assert p["fused_peb"] == (p["bwd_agg"] in (0, 1)), case
                # g_A (n,g,c) and g_sw (n,g) are carved exactly when a peb_bwd launch has to hand them over
                ws_rest.add(ws - (0 if p["fused_peb"] else al(4 * n * g * c) + al(4 * n * g)))
                # A (n,g,c) is saved exactly when the forward writes it
                saved_rest.add(saved - (al(4 * n * g * c) if p["keeps_A"] else 0))
                if p["fwd"] == F_TILE and not p["keeps_A"]:
                    assert saved == min(saved_rest), case
        # what is left is the same under every switch: nothing else in either carve follows them
        assert len(ws_rest) == 1 and len(saved_rest) == 1, (n, k, c, g, ws_rest, saved_rest)


def test_python_dropout_supported_follows_the_plan(L, monkeypatch):
    from ao_amd.ptv2 import gva

    checked = 0
    for env in ENVS:
        set_env(monkeypatch, env)
        for k, (g, c), n, drop, inv in shape_cases():
            if not gva.supported(c, g, k):
                continue
            got = describe(L, n, k, c, g, drop, inv)[F["bwd_takes_dropout"]]
            assert bool(got) == bool(gva.dropout_supported(c, g, k)), (env, n, k, c, g, drop, inv)
            checked += 1
    assert checked > 1000
