"""CPU: include/ptv2_octconv_hip.h, the eighteenth public header (OctFormer's dense octree convolutions), is exported by the built
library and bound from its text; its launchers refuse before any launch; OctFormer's state-dict keys; its registry entry."""
import ctypes
import os

import pytest


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    names = {"ptv2_octconv_abi_version", "ptv2_octconv_struct_bytes", "ptv2_octconv_workspace_bytes", "oct_conv_tables_hip_launcher",
             "oct_conv_fwd_hip_launcher", "oct_conv_gx_hip_launcher", "oct_conv_gw_hip_launcher"}
    assert set(_abi.octconv_signatures) == names
    with open(_abi.OCTCONV_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.octconv_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_octconv_abi_version() == _lib.EXPECTED_OCTCONV_ABI == 1
    sizes = [ctypes.sizeof(_abi.octconv_structs[k]) for k in ("octconv_args", "octconv_tables")]
    assert [L.ptv2_octconv_struct_bytes(i) for i in range(3)] == sizes + [-1]
    # ptv2_oct_hip.h is as it was
    assert L.ptv2_oct_abi_version() == 1 and L.ptv2_oct_struct_bytes(0) == ctypes.sizeof(_abi.oct_structs["oct_args"])
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert "ptv2_octconv_hip.h" in f.read(), "the build digest covers the header"


@pytest.mark.parametrize("cin,cout", [(10, 24), (24, 20), (24, 392), (388, 24), (0, 24)])
def test_launchers_refuse_unsupported_shapes_before_any_launch(cin, cout):
    """null operands: a launcher that went past its shape check would refuse for the pointers too, so the supported pair below
    shows that the shape alone decides the workspace query, and the launchers share its predicate"""
    from ao_amd import _abi, _lib

    L = _lib.lib()
    assert L.ptv2_octconv_workspace_bytes(40000, 27, 168, 168) == (8 * 27 * 168 + 64) * 168 * 4   # 8 partials of g_w, 64 strips of g_b
    assert L.ptv2_octconv_workspace_bytes(245, 8, 6, 24) == 64 * 24 * 4   # one split writes g_w itself
    assert L.ptv2_octconv_workspace_bytes(245, 27, cin, cout) == -1 and L.ptv2_octconv_workspace_bytes(245, 9, 24, 24) == -1
    a = _abi.octconv_structs["octconv_args"]()
    a.n_out, a.n_in, a.slots, a.cin, a.cout = 245, 245, 27, cin, cout
    for name in ("oct_conv_fwd_hip_launcher", "oct_conv_gx_hip_launcher", "oct_conv_gw_hip_launcher"):
        assert getattr(L, name)(ctypes.addressof(a), None) == 1, name   # PTV2_ERR_ARG
    assert L.oct_conv_tables_hip_launcher(ctypes.addressof(_abi.octconv_structs["octconv_tables"]()), None) == 1


def test_octformer_has_the_reference_state_dict_keys_and_shapes():
    """octformer_v1m1_base.py:368-563 with ocnn's names: OctreeConvBnRelu is .conv.weights (kdim, Cin, Cout) + .bn,
    OctreeDeconvBnRelu .deconv.weights (kdim, Cout, Cin) + .bn, Downsample .norm + .conv with a bias"""
    from ao_amd.octformer import OctFormer, OctreeDeconvBnRelu

    def bn(prefix, c):
        return {prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,), prefix + ".running_var": (c,),
                prefix + ".num_batches_tracked": ()}

    def conv_bn(prefix, kdim, cin, cout, conv="conv"):
        return dict(bn(prefix + ".bn", cout), **{prefix + "." + conv + ".weights": (kdim, cin, cout)})

    want = {}
    for i, (cin, cout) in enumerate(((6, 24), (48, 48))):
        want.update(conv_bn("patch_embed.convs.%d" % i, 27, cin, cout))
    for i, (cin, cout) in enumerate(((24, 48), (48, 96))):
        want.update(conv_bn("patch_embed.downsamples.%d" % i, 8, cin, cout))
    want.update(conv_bn("patch_embed.proj", 27, 96, 96))
    for i, (cin, cout) in enumerate(((96, 192), (192, 384), (384, 384))):
        want.update(bn("downsamples.%d.norm" % i, cout))
        want.update({"downsamples.%d.conv.weights" % i: (8, cin, cout), "downsamples.%d.conv.bias" % i: (cout,)})
    for i, c in enumerate((384, 384, 192, 96)):
        want.update({"decoder.conv1x1.%d.weight" % i: (168, c), "decoder.conv1x1.%d.bias" % i: (168,)})
        want.update(conv_bn("decoder.conv3x3.%d" % i, 27, 168, 168))
    for i in range(2):
        want.update(conv_bn("decoder.up_conv.%d" % i, 27, 168, 168, conv="deconv"))
    model = OctFormer(in_channels=6, num_classes=13)
    have = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.split(".")[0] in ("patch_embed", "downsamples", "decoder")}
    assert have == want
    assert tuple(OctreeDeconvBnRelu(16, 24, [3], 2, nempty=True).deconv.weights.shape) == (27, 24, 16)
    with pytest.raises(NotImplementedError):
        OctFormer(6, 13, nempty=False)
    with pytest.raises(ValueError):
        OctFormer(6, 13, octree_depth=7)   # 7 - 2 - 4 + 1 = 2 is not above octree_full_depth


def test_registry_files_octformer_and_returns_the_same_list():
    import ao_amd.ptv2.registry as registry
    from ao_amd.octformer import OctFormer

    class Fake:
        def __init__(self):
            self.entries = {}

        def register_module(self, module, name, force=False):
            self.entries[name] = module

    models = Fake()
    assert registry.register(MODELS=models) == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image"]
    assert models.entries["OctFormer-v1m1"] is OctFormer
