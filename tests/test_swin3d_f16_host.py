"""CPU: include/ptv2_swin_f16_hip.h, the seventeenth public header (Swin3D's window attention on half-precision storage), is
exported by the built library and bound from its text; no compute calls."""
import ctypes
import os


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    names = {"ptv2_swin_f16_abi_version", "ptv2_swin_f16_struct_bytes", "ptv2_swin_f16_workspace_bytes",
             "ptv2_swin_f16_fwd_resident_blocks", "swin_attention_f16_fwd_hip_launcher", "swin_attention_f16_bwd_hip_launcher"}
    assert set(_abi.swin_f16_signatures) == names
    with open(_abi.SWIN_F16_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.swin_f16_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_swin_f16_abi_version() == _lib.EXPECTED_SWIN_F16_ABI == 1
    args = _abi.swin_f16_structs["swin_f16_args"]
    assert L.ptv2_swin_f16_struct_bytes(0) == ctypes.sizeof(args) and L.ptv2_swin_f16_struct_bytes(1) == -1
    assert _abi.swin_f16_consts["SWIN_F16_MAX_GROUPS"] == _abi.swin_consts["SWIN_MAX_GROUPS"]
    # ptv2_swin_hip.h is as it was
    assert L.ptv2_swin_abi_version() == 1 and L.ptv2_swin_struct_bytes(0) == ctypes.sizeof(_abi.swin_structs["swin_args"])
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert "ptv2_swin_f16_hip.h" in f.read(), "the build digest covers the header"


def test_launchers_refuse_unsupported_shapes_before_any_launch():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    assert L.ptv2_swin_f16_workspace_bytes(1000, 10, 6, 16, 312) == L.ptv2_swin_workspace_bytes(1000, 10, 6, 16, 312) > 0
    for n, windows, h, hd, rows in ((1000, 10, 6, 12, 312), (1000, 10, 65, 8, 312), (1000, 10, 6, 16, 402), (10, 11, 6, 16, 312)):
        assert L.ptv2_swin_f16_workspace_bytes(n, windows, h, hd, rows) == -1
    assert L.ptv2_swin_f16_fwd_resident_blocks(12, 3, 312) == L.ptv2_swin_f16_fwd_resident_blocks(16, 3, 402) == -1
    a = _abi.swin_f16_structs["swin_f16_args"]()   # zeroed: no groups
    assert L.swin_attention_f16_fwd_hip_launcher(ctypes.addressof(a), None) == 1   # PTV2_ERR_ARG
    assert L.swin_attention_f16_bwd_hip_launcher(ctypes.addressof(a), None) == 1
