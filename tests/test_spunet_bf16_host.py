"""CPU: the thirteenth header (include/ptv2_spconv_bf16_hip.h: the bf16-operand sparse convolutions of ao_amd/csrc/spconv_bf16.hip).
It parses through ao_amd/_abi.py; its symbols are in the built library with the declared arity; the ABI version is 1; the
workspace function refuses bad arguments and stops growing with n; the launchers refuse a shape outside the contract with a
status before anything is enqueued.  Every test here fails on the parent commit: the header and the symbols do not exist there."""
import re

NAMES = ("ptv2_spconv_bf16_abi_version", "ptv2_spconv_bf16_workspace_bytes", "spconv_bf16_conv_hip_launcher",
         "spconv_bf16_wgrad_hip_launcher")


def test_header_parses_and_the_symbols_have_the_declared_arity():
    from ao_amd import _abi, _lib

    assert set(NAMES) == set(_abi.spconv_bf16_signatures)
    txt = re.sub(r"/\*.*?\*/", "", open(_abi.SPCONV_BF16_HEADER).read(), flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        declared = len([a for a in m.group(1).split(",") if a.strip() not in ("", "void")])
        assert len(getattr(L, name).argtypes) == declared == len(_abi.spconv_bf16_signatures[name][1]), name
    assert L.ptv2_spconv_bf16_abi_version() == _lib.EXPECTED_SPCONV_BF16_ABI == 1


def test_workspace_bytes():
    from ao_amd import _abi, _lib

    ws = _lib.lib().ptv2_spconv_bf16_workspace_bytes
    for n, k, cin, cout in ((-1, 27, 32, 32), (10, 0, 32, 32), (10, 28, 32, 32), (10, 27, 48, 32), (10, 27, 32, 16), (10, 8, 8192, 32)):
        assert ws(n, k, cin, cout) == -1, (n, k, cin, cout)
    one = 27 * 128 * 96
    assert ws(0, 27, 128, 96) == ws(1024, 27, 128, 96) >= 2 * one + 4 * one  # the packed weight and one split of partial sums
    assert ws(1025, 27, 128, 96) - ws(1024, 27, 128, 96) == 4 * one
    top = 1024 * _abi.spconv_consts["SPCONV_MAX_SPLITS"]
    assert ws(top, 27, 128, 96) == ws(100 * top, 27, 128, 96) < 2 * one + 4 * one * 8 + 1024


def test_launchers_refuse_shapes_outside_the_contract():
    from ao_amd import _abi, _lib

    L, p = _lib.lib(), 4096  # (never dereferenced: the status comes before anything is enqueued)
    gather, scatter = _abi.spconv_consts["SPCONV_GATHER"], _abi.spconv_consts["SPCONV_SCATTER"]
    for form, k, cin, cout, reverse in ((gather, 27, 48, 32, 0), (gather, 28, 32, 32, 0), (scatter, 8, 32, 32, 1), (2, 8, 32, 32, 0)):
        rc = L.spconv_bf16_conv_hip_launcher(form, 100, 100, k, cin, cout, p, p, p, 0, reverse, p, p, 1 << 30, 0)
        assert rc == 1, (form, k, cin, cout, reverse, rc)
    for k, cin, cout in ((27, 48, 32), (28, 32, 32), (27, 32, 80)):
        assert L.spconv_bf16_wgrad_hip_launcher(100, 100, k, cin, cout, p, p, p, 0, p, p, 1 << 30, 0) == 1, (k, cin, cout)
    # a short workspace is PTV2_ERR_WORKSPACE, also before anything is enqueued
    assert L.spconv_bf16_conv_hip_launcher(gather, 100, 100, 27, 32, 32, p, p, p, 0, 0, p, p, 64, 0) == 2
    assert L.spconv_bf16_wgrad_hip_launcher(100, 100, 27, 32, 32, p, p, p, 0, p, p, 64, 0) == 2
