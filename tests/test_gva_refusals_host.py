"""CPU: the public attention launchers refuse bad arguments with the code, and at the point, they always did.

Every case below is rejected by a check that sits in front of the first HIP call of its path (read in gva_aggregate.hip and
gva_block.hip; gva_plan() and the attention-dropout setting are host code), so the calls need no device: every pointer is
the address of one small host buffer that is never dereferenced.  The expected codes were recorded from the library of the
commit before the internal interfaces took operand bundles (gva_common.h: AttnIn ...), and the file passes against both.

Three cases are not listed in their obvious form, because the obvious form is not a refusal (or does not exist):
  * gva_block_workspace_bytes() includes 1024 bytes that the launchers' own check does not ask for, so a workspace one byte
    short of it is accepted; refused is one byte short of what the check asks for, gva_block_workspace_bytes() - 1024.
  * attn_drop_p outside [0, 1] is checked by gva_block_forward_hip_launcher only (the backward clamps it).
  * `g_A set, g_sw NULL` exists for gva_aggregate_backward_hip_launcher alone: the other two take neither.
"""
import ctypes

import pytest

ERR_ARG, ERR_WORKSPACE = 1, 2
SWITCHES = ("AO_AMD_FWD_STAGED", "AO_AMD_BWD_STAGED", "AO_AMD_BWD_POINT", "AO_AMD_TILE_KEEP_A", "AO_AMD_LOGITS_BWD")
GOOD = (130, 16, 96, 12)  # (n, k, c, g) with an instance of every form


@pytest.fixture(scope="module")
def L():
    import os

    from ao_amd import _lib
    import ao_amd.ptv2.gva  # noqa: F401  (the struct mirrors are checked against the library)

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def dummy():
    buf = ctypes.create_string_buffer(256)
    yield ctypes.addressof(buf)
    del buf


def agg_forward(L, p, n, k, c, g):
    return L.gva_aggregate_forward_hip_launcher(n, k, c, g, *([p] * 14), 0)


# pointer arguments behind (n, k, c, g): 10 inputs, w, g_out, g_A, g_sw | Wp2, bp2, inv_ptr, inv_rows, 8 outputs
def agg_backward(L, p, n, k, c, g, g_sw=True, workspace=True, workspace_bytes=1 << 40):
    ptrs = [p] * 24
    if not g_sw:
        ptrs[13] = None
    return L.gva_aggregate_backward_hip_launcher(n, k, c, g, *ptrs, p if workspace else None, workspace_bytes, 0)


def attn_backward(L, p, n, k, c, g, workspace=True, workspace_bytes=1 << 40):
    return L.gva_attention_backward_hip_launcher(n, k, c, g, *([p] * 24), p if workspace else None, workspace_bytes, 0)


BAD_SHAPES = [(-1, 16, 96, 12), (130, 12, 96, 12), (130, 16, 50, 6)]  # n = -1; k = 12; (c, g) = (50, 6)


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_stage_launchers_refuse_bad_shapes(L, dummy, shape):
    assert agg_forward(L, dummy, *shape) == ERR_ARG
    assert agg_backward(L, dummy, *shape) == ERR_ARG
    assert attn_backward(L, dummy, *shape) == ERR_ARG


def test_aggregate_backward_refuses_g_A_without_g_sw(L, dummy):
    assert agg_backward(L, dummy, *GOOD, g_sw=False) == ERR_ARG


@pytest.mark.parametrize("call", [agg_backward, attn_backward])
def test_backward_refuses_a_missing_or_short_workspace(L, dummy, call):
    need = L.gva_aggregate_workspace_bytes(*GOOD)
    assert need > 0
    assert call(L, dummy, *GOOD, workspace=False) == ERR_WORKSPACE
    assert call(L, dummy, *GOOD, workspace_bytes=need - 1) == ERR_WORKSPACE


def block_args(p, n, k, c, g, attn_drop_p=0.0):
    from ao_amd import _abi

    B, G = _abi.structs["ptv2_gva_block"](), _abi.structs["ptv2_gva_block_grads"]()
    for S in (B, G):
        for name, kind in S._fields_:
            if kind is ctypes.c_void_p:
                setattr(S, name, p)
    B.n, B.k, B.c, B.g, B.training = n, k, c, g, 1
    B.eps_p = B.eps_w = 1e-5
    B.momentum_p = B.momentum_w = 0.1
    B.attn_drop_p, B.attn_drop_seed = attn_drop_p, 7
    return B, G


def block_forward(L, B, p, workspace_bytes=1 << 40):
    return L.gva_block_forward_hip_launcher(ctypes.addressof(B), p, workspace_bytes, 0)


def block_backward(L, B, G, p, workspace_bytes=1 << 40):
    return L.gva_block_backward_hip_launcher(ctypes.addressof(B), ctypes.addressof(G), p, workspace_bytes, 0)


def test_block_forward_refuses_attn_drop_p_out_of_range(L, dummy):
    B, _ = block_args(dummy, *GOOD, attn_drop_p=1.5)
    assert block_forward(L, B, dummy) == ERR_ARG


def test_block_launchers_refuse_c_not_a_multiple_of_g(L, dummy):
    B, G = block_args(dummy, 130, 16, 50, 6)
    assert block_forward(L, B, dummy) == ERR_ARG
    assert block_backward(L, B, G, dummy) == ERR_ARG


def test_block_launchers_refuse_a_short_workspace(L, dummy):
    B, G = block_args(dummy, *GOOD)
    need = L.gva_block_workspace_bytes(*GOOD) - 1024  # (what the launchers check: the public figure has 1024 bytes to spare)
    assert need > 0
    assert block_forward(L, B, dummy, workspace_bytes=need - 1) == ERR_WORKSPACE
    assert block_backward(L, B, G, dummy, workspace_bytes=need - 1) == ERR_WORKSPACE
