"""CPU: include/ptv2_octconv_bf16_hip.h, the nineteenth public header (OctFormer's octree convolutions with bf16 matrix-core
operands), is exported by the built library and bound from its text; its launchers refuse before any launch; ptv2_octconv_hip.h
is as it was; conv_operands reaches every convolution and leaves the state dict alone."""
import ctypes
import os

import pytest

LAUNCHERS = ("oct_conv_bf16_fwd_hip_launcher", "oct_conv_bf16_gx_hip_launcher", "oct_conv_bf16_gw_hip_launcher")


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    assert set(_abi.octconv_bf16_signatures) == {"ptv2_octconv_bf16_abi_version", "ptv2_octconv_bf16_workspace_bytes"} | set(LAUNCHERS)
    with open(_abi.OCTCONV_BF16_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.octconv_bf16_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_octconv_bf16_abi_version() == _lib.EXPECTED_OCTCONV_BF16_ABI == 1
    assert not _abi.octconv_bf16_consts and L.ptv2_octconv_abi_version() == 1
    old, new = _abi.octconv_structs["octconv_args"], _abi.octconv_bf16_structs["octconv_bf16_args"]
    assert [(n, t) for n, t in old._fields_] == [(n, t) for n, t in new._fields_] and ctypes.sizeof(old) == ctypes.sizeof(new)
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert "ptv2_octconv_bf16_hip.h" in f.read(), "the build digest covers the header"


@pytest.mark.parametrize("cin,cout", [(6, 24), (8, 24), (10, 24), (24, 20), (24, 392), (388, 24), (0, 24)])
def test_launchers_refuse_unsupported_shapes_before_any_launch(cin, cout):
    """the fp32 set without the stem; null operands, so the supported pair shows that the shape alone decides the query"""
    from ao_amd import _abi, _lib

    L = _lib.lib()
    assert L.ptv2_octconv_bf16_workspace_bytes(40000, 27, 168, 168) == L.ptv2_octconv_workspace_bytes(40000, 27, 168, 168) > 0
    assert L.ptv2_octconv_bf16_workspace_bytes(245, 27, cin, cout) == -1 and L.ptv2_octconv_bf16_workspace_bytes(245, 9, 24, 24) == -1
    a = _abi.octconv_bf16_structs["octconv_bf16_args"]()
    for name in LAUNCHERS:
        assert getattr(L, name)(ctypes.addressof(a), None) == 1, name   # PTV2_ERR_ARG on a zeroed struct
    a.n_out, a.n_in, a.slots, a.cin, a.cout = 245, 245, 27, cin, cout
    for name in LAUNCHERS:
        assert getattr(L, name)(ctypes.addressof(a), None) == 1, name


def test_conv_operands_reaches_every_convolution_and_no_state_dict_key():
    from ao_amd.octformer import OctFormer
    from ao_amd.octformer.model import OctreeConv

    plain, bf16 = OctFormer(6, 13), OctFormer(6, 13, conv_operands="bf16")
    assert [m.operands for m in bf16.modules() if isinstance(m, OctreeConv)] == ["bf16"] * 14
    assert {k: v.shape for k, v in plain.state_dict().items()} == {k: v.shape for k, v in bf16.state_dict().items()}
    with pytest.raises(ValueError, match="conv_operands"):
        OctFormer(6, 13, conv_operands="fp16")
