"""CPU: the contract of SpUNet-v1m1's sparse convolutions against dense torch convolutions, and the host
side of ao_amd/spunet and include/ptv2_spconv_hip.h."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spunet_cases as SC
from tests import spunet_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-12


def _grid_case(clouds, side, seed):
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    coord = np.concatenate([cells[rng.permutation(cells.shape[0])[:c]] for c in clouds]).astype(np.int32)
    return coord, np.cumsum(clouds).astype(np.int32)


def _dense(x, coord, offset, side):
    """(b, C, side, side, side) with the rows of x at their voxels"""
    cloud = np.searchsorted(offset, np.arange(coord.shape[0]), side="right")
    out = x.new_zeros((len(offset), x.shape[1], side, side, side))
    out[cloud, :, coord[:, 0], coord[:, 1], coord[:, 2]] = x
    return out


def _rows(dense, coord, offset):
    cloud = np.searchsorted(offset, np.arange(coord.shape[0]), side="right")
    return dense[cloud, :, coord[:, 0], coord[:, 1], coord[:, 2]]


# a 12^3 grid with 150 voxels, and two clouds on one grid
@pytest.mark.parametrize("clouds", [(150,), (90, 40)])
def test_table_forms_equal_the_dense_convolutions(clouds):
    side, cin, cout = 12, 5, 7
    coord, offset = _grid_case(clouds, side, 11)
    t = R.tables_to(R.build_tables(coord, offset, levels=2), "cpu")
    g = torch.Generator().manual_seed(3)
    x = torch.randn((coord.shape[0], cin), generator=g, dtype=torch.float64)
    scale = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    for k, tab in ((3, t["nbr3"][0]), (5, t["nbr5"])):
        w = torch.randn((cout, k, k, k, cin), generator=g, dtype=torch.float64)
        dense = F.conv3d(_dense(x, coord, offset, side), w.permute(0, 4, 1, 2, 3), padding=k // 2)
        assert scale(R.gather(x, tab, w), _rows(dense, coord, offset)) <= TOL, k
        # the reversal symmetry: j = nbr[i, kappa]  <=>  i = nbr[j, K - 1 - kappa]
        tab = tab.numpy()
        i, kappa = np.nonzero(tab >= 0)
        assert np.array_equal(tab[tab[i, kappa], tab.shape[1] - 1 - kappa], i)
    # stride 2: outputs at every coarse voxel with a child, zero elsewhere
    w = torch.randn((cout, 2, 2, 2, cin), generator=g, dtype=torch.float64)
    dense = F.conv3d(_dense(x, coord, offset, side), w.permute(0, 4, 1, 2, 3), stride=2)
    ccoord, coffset = t["coord"][1].numpy(), t["offset"][1].numpy()
    down = R.gather(x, t["child"][0], w)
    assert scale(down, _rows(dense, ccoord, coffset)) <= TOL
    assert int((dense.abs().sum(1) > 0).sum()) <= ccoord.shape[0] and float(dense.abs().sum()) > 0
    assert scale(_dense(down, ccoord, coffset, side // 2), dense) <= TOL, "no output outside the coarse voxels"
    # the coarse rows ascend in (cloud, x, y, z)
    ccloud = np.searchsorted(coffset, np.arange(ccoord.shape[0]), side="right")
    keys = [tuple(v) for v in np.concatenate([ccloud[:, None], ccoord], 1)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # inverse: conv_transpose3d(stride 2) read at the fine voxels
    y = torch.randn((ccoord.shape[0], cin), generator=g, dtype=torch.float64)
    dense = F.conv_transpose3d(_dense(y, ccoord, coffset, side // 2), w.permute(4, 0, 1, 2, 3), stride=2)
    assert scale(R.scatter(y, t["child"][0], w, coord.shape[0]), _rows(dense, coord, offset)) <= TOL
    # parent / slot are child the other way
    child, parent, slot = t["child"][0].numpy(), t["parent"][0].numpy(), t["slot"][0].numpy()
    assert np.array_equal(child[parent, slot], np.arange(coord.shape[0])) and int((child >= 0).sum()) == coord.shape[0]


def test_manifest_and_strict_loading():
    from ao_amd import spunet

    with open(os.path.join(GOLDEN, "spunet_manifest.json")) as f:
        manifest = json.load(f)
    assert set(manifest) == {"num_classes_13", "num_classes_0"}
    for classes in (13, 0):
        want = manifest["num_classes_%d" % classes]
        model = spunet.SpUNetBase(6, classes)
        have = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert have == want, classes
        assert list(have) == list(want), "the reference's key order"
        ref = R.SpUNet(6, classes)
        assert {k: list(v.shape) for k, v in ref.state_dict().items()} == want
        state = SC.fill_state(SC.shapes_of(ref), 3)
        ref.load_state_dict(state, strict=True)
        model.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(model.state_dict(), strict=True)
        for key, value in model.state_dict().items():
            assert torch.equal(value, state[key]), key
    assert len(manifest["num_classes_13"]) == 356 and len(manifest["num_classes_0"]) == 354
    assert want["conv_input.0.weight"] == [32, 5, 5, 5, 6] and want["up.0.0.weight"] == [96, 2, 2, 2, 96]
    assert manifest["num_classes_13"]["final.weight"] == [13, 1, 1, 1, 96]
    assert sum(p.numel() for p in spunet.SpUNetBase(6, 13).parameters()) == 39157165


def test_constructor_and_init():
    from ao_amd import spunet

    with pytest.raises(NotImplementedError):
        spunet.SpUNetBase(6, 13, cls_mode=True)
    model = spunet.SpUNetBase(4, 20, base_channels=32, channels=(32, 64, 64, 32), layers=(1, 1, 1, 1))
    assert model.num_stages == 2 and tuple(model.final.weight.shape) == (20, 1, 1, 1, 32)
    assert float(model.final.bias.detach().abs().max()) == 0.0
    w = model.enc[0].block0.conv1.weight
    assert abs(float(w.detach().std()) - 0.02) < 0.002 and float(w.detach().abs().max()) < 0.2  # trunc_normal_(std=0.02), cut at +-2
    for bn in (model.conv_input[1], model.down[0][1]):
        assert float(bn.weight.detach().min()) == 1.0 and float(bn.bias.detach().abs().max()) == 0.0 and bn.eps == 1e-3 and bn.momentum == 0.01
    d = model.down[0][0].weight  # spconv's default: U(+-1 / sqrt(8 Cin))
    assert 0.9 / np.sqrt(8 * 32) < float(d.detach().abs().max()) <= 1.0 / np.sqrt(8 * 32)


def test_registry_files_the_name():
    from ao_amd import spunet
    from ao_amd.ptv2 import registry

    class Fake:
        def __init__(self):
            self.modules = {}

        def register_module(self, module=None, name=None, force=False):
            self.modules[name] = module

    fake = Fake()
    done = registry.register(MODELS=fake)
    assert done == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image"]
    assert fake.modules["SpUNet-v1m1"] is spunet.SpUNetBase
    assert fake.modules["SpUNet-v1m1"](in_channels=6, num_classes=0).num_classes == 0


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    names = {"ptv2_spconv_abi_version", "ptv2_spconv_struct_bytes", "ptv2_spconv_tables_workspace_bytes",
             "ptv2_spconv_workspace_bytes", "spconv_build_tables_hip_launcher", "spconv_conv_hip_launcher",
             "spconv_wgrad_hip_launcher", "spconv_stem_hip_launcher"}
    assert set(_abi.spconv_signatures) == names
    with open(_abi.SPCONV_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.spconv_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_spconv_abi_version() == _lib.EXPECTED_SPCONV_ABI == 1
    assert L.ptv2_spconv_struct_bytes(0) == ctypes.sizeof(_abi.spconv_structs["spconv_tables"]) == 8 * (1 + 5 + 5 * 4 + 2)
    assert L.ptv2_spconv_struct_bytes(1) == -1
    # the other headers are as they were
    assert _lib.EXPECTED_ABI == 11 and L.ptv2_abi_version() == 11 and L.ptv2_ptv1_abi_version() == 1


def test_memory_rule():
    """no n * K * C buffer: the workspace of every convolution of a 100 000-voxel scene's five levels is the weight gradient's
    partial sums -- K * splits * Cout * Cin floats, at most SPCONV_MAX_SPLITS splits -- so it stays below one (n, K, Cin) fp32
    tensor at the full-resolution level, and at every level it stops growing once the splits are used up"""
    from ao_amd import _abi, _lib

    L = _lib.lib()
    splits = _abi.spconv_consts["SPCONV_MAX_SPLITS"]
    # (rows, K, Cin, Cout): the widest convolution of each level of SpUNet-v1m1; the rows of a typical indoor scene
    levels = ((100000, 27, 128, 96), (100000, 125, 6, 32), (30000, 27, 192, 128), (8000, 27, 384, 256), (2000, 27, 256, 256),
              (500, 27, 256, 256), (30000, 8, 32, 64), (500, 8, 256, 256))
    for n, k, cin, cout in levels:
        ws = L.ptv2_spconv_workspace_bytes(n, k, cin, cout)
        assert 0 < ws <= 4 * k * splits * cin * cout + 256, (n, k, cin, cout, ws)
        assert L.ptv2_spconv_workspace_bytes(100 * n, k, cin, cout) <= 4 * k * splits * cin * cout + 256
        assert L.ptv2_spconv_workspace_bytes(10 ** 7, k, cin, cout) == L.ptv2_spconv_workspace_bytes(10 ** 8, k, cin, cout)
    n, k, cin, cout = levels[0]
    assert L.ptv2_spconv_workspace_bytes(n, k, cin, cout) < 4 * n * k * cin // 10
    for bad in ((-1, 27, 32, 32), (100, 0, 32, 32), (100, 126, 32, 32), (100, 27, 0, 32), (100, 27, 32, 0)):
        assert L.ptv2_spconv_workspace_bytes(*bad) == -1
    # the table build: integer tables only, a fixed number of words per row
    assert 0 < L.ptv2_spconv_tables_workspace_bytes(100000, 2) <= 100000 * 8 * 12 + (1 << 22)
    assert L.ptv2_spconv_tables_workspace_bytes(0, 1) == -1 and L.ptv2_spconv_tables_workspace_bytes(10, 2000) == -1


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_no_cpu_fallback(path, monkeypatch):
    from ao_amd import spunet

    monkeypatch.setenv("AO_AMD_SPUNET", path)
    batch = {k: torch.from_numpy(v) for k, v in SC.model_batch().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spunet.build_tables(batch["discrete_coord"], batch["offset"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spunet.SpUNetBase(6, 13)(batch)
    with pytest.raises(TypeError, match="build_tables"):
        spunet.subm_conv(torch.zeros(4, 32), torch.zeros(32, 3, 3, 3, 32), {"nbr3": None}, 0)
    with pytest.raises(TypeError):
        spunet.SpconvTables(None)


def test_the_model_batch_is_the_designed_one():
    batch = SC.model_batch()
    t = R.build_tables(batch["discrete_coord"], batch["offset"])
    assert batch["offset"].tolist() == [2130, 3424] and t["n"] == [3424, 983, 248, 61, 10]
    assert len({tuple(v) for v in batch["discrete_coord"][:2130]}) == 2130
