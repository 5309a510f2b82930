"""GPU: ao_amd.octformer's operators (ao_amd/csrc/oct_attention.hip, oct_dwconv.hip) against tests/octformer_ref.py.

Against float64: out, g_qkv and g_table of octree_attention over the cases of tests/octformer_cases.py, and y, g_x, g_w of
octree_dwconv at C in {96, 16}; the compared key set is asserted.  The bound is the rule of tests/test_gpu_st_ops.py:
e_kernel <= M[key] * max(e_eager, 2^-24) in relative L2, e_eager the distance from float64 of the fp32 run of octformer_ref on
the same device and inputs.  M per key: twice the worst ratio measured on the MI355X over all cases, rounded up to a power of
two.

Exact: the neighbour table against a dictionary-built one; two runs give the same bits for out, g_qkv, y, g_x and g_w; a shape
outside the supported set raises ValueError."""
import numpy as np
import pytest
import torch

from tests import octformer_cases as OC
from tests import octformer_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
ATTN_KEYS = {"out", "g_qkv", "g_table"}
CONV_KEYS = {"y", "g_x", "g_w"}
# M per key: 2 x the worst e_kernel / max(e_eager, 2^-24) over every case, as a power of two
M = {"out": 4, "g_qkv": 4, "g_table": 8, "y": 2, "g_x": 2, "g_w": 4}

_REF = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def check(tag, res, f64, f32, keys):
    assert set(res) == keys and set(f64) == keys and set(f32) == keys
    bad = []
    for key in sorted(keys):
        assert torch.isfinite(res[key]).all(), key
        got, eager = _l2(res[key], f64[key]), _l2(f32[key], f64[key])
        print("oct-ratio %-24s %-8s kernel %.3e  eager %.3e  ratio %.3f" % (tag, key, got, eager, got / max(eager, FLOOR)))
        if not got <= M[key] * max(eager, FLOOR):
            bad.append((key, got, M[key] * max(eager, FLOOR)))
    assert not bad, bad


def dict_neighbours(xyz, batch):
    """(n, 27) from a dictionary of (cloud, x, y, z)"""
    rows = {(b,) + tuple(p): i for i, (b, p) in enumerate(zip(batch.tolist(), xyz.tolist()))}
    return np.array([[rows.get((b, x + dx, y + dy, z + dz), -1) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
                     for b, (x, y, z) in zip(batch.tolist(), xyz.tolist())], np.int32)


def level_of(xyz, batch):
    from ao_amd.octformer import octree_level

    return octree_level(_dev(xyz), _dev(batch), OC.DEPTH)


# ------------------------------------------------------------------------------------------------------- exact ----
def test_neighbour_table_equals_the_dictionary():
    """per cloud: a dense 4 x 4 x 4 block, an isolated voxel, voxels at 0 and at 2^depth - 1 on every axis pattern (a key that
    wrapped would find them); two clouds on identical coordinates; rows given in a shuffled order"""
    top = 2 ** OC.DEPTH - 1
    block = np.stack(np.meshgrid(*[np.arange(10, 14)] * 3, indexing="ij"), -1).reshape(-1, 3)
    corners = np.array([[a, b, c] for a in (0, top) for b in (0, top) for c in (0, top)])
    one = np.concatenate([block, [[100, 100, 100]], corners]).astype(np.int64)
    xyz, batch = np.concatenate([one, one]), np.repeat([0, 1], len(one))
    perm = np.random.default_rng(3).permutation(len(xyz))
    level = level_of(xyz[perm], batch[perm])
    sx, sb = level.xyz.cpu().numpy(), level.batch.cpu().numpy()
    assert np.array_equal(sx, xyz[perm][level.order.cpu().numpy()]) and np.array_equal(sb, np.sort(batch))
    assert np.array_equal(np.lexsort((OC.morton(sx[:, 0], sx[:, 1], sx[:, 2]), sb)), np.arange(len(sb)))
    nbr = level.nbr.cpu().numpy()
    assert np.array_equal(nbr, dict_neighbours(sx, sb))
    lone = np.flatnonzero((sx == 100).all(1))
    assert len(lone) == 2 and all((nbr[i] >= 0).sum() == 1 and nbr[i, 13] == i for i in lone)


@pytest.mark.parametrize("name", sorted(OC.ATTENTION))
def test_neighbour_table_of_the_attention_clouds(name):
    t = OC.attention_inputs(name)
    level = level_of(t["xyz"], t["batch"])
    assert torch.equal(level.order.cpu(), torch.arange(len(t["xyz"])))   # the cases are in node order already
    assert np.array_equal(level.nbr.cpu().numpy(), dict_neighbours(t["xyz"], t["batch"]))


def test_octree_level_refuses_duplicates_and_coordinates_outside_the_cube():
    from ao_amd.octformer import octree_level

    with pytest.raises(ValueError):
        octree_level(_dev(np.array([[1, 2, 3], [1, 2, 3]])), _dev(np.array([0, 0])), 9)
    with pytest.raises(ValueError):
        octree_level(_dev(np.array([[1, 2, 512]])), _dev(np.array([0])), 9)


# ------------------------------------------------------------------------------------------ against float64 ----
def run_attention(name, fn, dtype):
    _, K, D, H, hd = OC.ATTENTION[name]
    t = OC.attention_inputs(name)
    qkv, table = (_dev(t[k]).to(dtype).requires_grad_(True) for k in ("qkv", "table"))
    out = fn(qkv, table, K, D, hd ** -0.5)
    g_qkv, g_table = torch.autograd.grad(out, (qkv, table), _dev(t["g_out"]).to(dtype))
    return {"out": out.detach(), "g_qkv": g_qkv, "g_table": g_table}


def attention_reference(name):
    if ("attn", name) not in _REF:
        t = OC.attention_inputs(name)
        xyz, batch, clouds = _dev(t["xyz"]), _dev(t["batch"]), int(t["batch"].max()) + 1
        _REF[("attn", name)] = tuple(run_attention(name, lambda qkv, table, K, D, s: R.attention(qkv, xyz, batch, clouds, table, K, D, s), dt)
                                     for dt in (torch.float64, torch.float32))
    return _REF[("attn", name)]


def our_attention(name):
    from ao_amd.octformer import octree_attention

    t = OC.attention_inputs(name)
    level = level_of(t["xyz"], t["batch"])
    return run_attention(name, lambda qkv, table, K, D, s: octree_attention(qkv, level, table, K, D, s), torch.float32)


@pytest.mark.parametrize("name", sorted(OC.ATTENTION))
def test_octree_attention_against_float64(name):
    f64, f32 = attention_reference(name)
    check(name, our_attention(name), f64, f32, ATTN_KEYS)


def run_dwconv(C, fn, dtype):
    xyz, batch = OC.cloud((100, 145), seed=7)
    rng = np.random.default_rng(C)
    x, w = (_dev(rng.standard_normal(s).astype(np.float32)).to(dtype).requires_grad_(True) for s in ((len(xyz), C), (27, 1, C)))
    y = fn(x, w, xyz, batch)
    g_x, g_w = torch.autograd.grad(y, (x, w), _dev(rng.standard_normal((len(xyz), C)).astype(np.float32)).to(dtype))
    return {"y": y.detach(), "g_x": g_x, "g_w": g_w}


def our_dwconv(C):
    from ao_amd.octformer import octree_dwconv

    return run_dwconv(C, lambda x, w, xyz, batch: octree_dwconv(x, w, level_of(xyz, batch)), torch.float32)


@pytest.mark.parametrize("C", [96, 16])
def test_octree_dwconv_against_float64(C):
    f64, f32 = (run_dwconv(C, lambda x, w, xyz, batch: R.dwconv(x, w, _dev(dict_neighbours(xyz, batch))), dt)
                for dt in (torch.float64, torch.float32))
    check("dwconv-%d" % C, our_dwconv(C), f64, f32, CONV_KEYS)


# ------------------------------------------------------------------------------------- repeatability, limits ----
def test_two_runs_give_the_same_bits():
    a, b = our_attention("two-clouds-dilated"), our_attention("two-clouds-dilated")
    assert all(torch.equal(a[k], b[k]) for k in ("out", "g_qkv"))
    a, b = our_dwconv(96), our_dwconv(96)
    assert all(torch.equal(a[k], b[k]) for k in ("y", "g_x", "g_w"))


@pytest.mark.parametrize("K,D,H,hd", [(33, 1, 6, 16), (26, 4, 6, 8), (26, 4, 65, 16), (26, 0, 6, 16), (32, 25, 6, 16)],
                         ids=["patch-33", "hd-8", "heads-65", "dilation-0", "rpe-257"])
def test_attention_outside_the_supported_shapes_raises(K, D, H, hd):
    from ao_amd.octformer import octree_attention

    xyz, batch = OC.cloud((19,), seed=1)
    R_ = 2 * int(0.8 * K * max(D, 1) ** 0.5) + 1
    with pytest.raises(ValueError):
        octree_attention(torch.zeros(19, 3 * H * hd, device="cuda"), level_of(xyz, batch), torch.zeros(3 * R_, H, device="cuda"), K, D, 0.25)


@pytest.mark.parametrize("C", [18, 1028])
def test_dwconv_outside_the_supported_channels_raises(C):
    from ao_amd.octformer import octree_dwconv

    xyz, batch = OC.cloud((19,), seed=1)
    with pytest.raises(ValueError):
        octree_dwconv(torch.zeros(19, C, device="cuda"), torch.zeros(27, 1, C, device="cuda"), level_of(xyz, batch))
