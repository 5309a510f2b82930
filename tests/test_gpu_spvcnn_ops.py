"""GPU: ao_amd.spvcnn's map and operators (ao_amd/csrc/spv_map.hip, spv_ops.hip) against tests/spvcnn_ref.py on the batch of
tests/spvcnn_cases.py at levels 0, 2 and 4: devoxelize at C in {32, 96, 256}, voxelize also at C = 6.  The bound is the rule of
tests/test_gpu_octformer_ops.py: e_kernel <= M[key] * max(e_eager, 2^-24) in relative L2 against float64, e_eager the fp32 run of
spvcnn_ref on the same device and inputs; M per key is twice the worst ratio measured on the MI355X over all cases, rounded up to
a power of two.  Exact: row, counts and CSR of every level against the dictionary; two runs give the same
bits; level 0 is the gather F[row[0]]; an unsupported width raises ValueError."""
import functools

import numpy as np
import pytest
import torch

from tests import spvcnn_cases as SC
from tests import spvcnn_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
DEVOX_KEYS = {"out", "g_feat", "g_add"}
VOX_KEYS = {"v", "g_x"}
# M per key: 2 x the worst e_kernel / max(e_eager, 2^-24) over every case, as a power of two
M = {"out": 2, "g_feat": 4, "g_add": 1, "v": 2, "g_x": 1}

@functools.lru_cache(None)
def geometry():
    return R.Geometry(*SC.batch(), device="cuda")


@functools.lru_cache(None)
def pvmap():
    from ao_amd.spvcnn import point_voxel_map

    return point_voxel_map(*(torch.from_numpy(a).cuda() for a in SC.batch()))


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def check(tag, res, f64, f32, keys, bound=None):
    assert set(res) == keys and set(f64) == keys and set(f32) == keys
    bound = bound or M.get
    bad = []
    for key in sorted(keys):
        assert torch.isfinite(res[key]).all(), key
        got, eager = _l2(res[key], f64[key]), _l2(f32[key], f64[key])
        print("spv-ratio %-16s %-8s kernel %.3e  eager %.3e  ratio %.3f" % (tag, key, got, eager, got / max(eager, FLOOR)))
        if not got <= bound(key) * max(eager, FLOOR):
            bad.append((key, got, bound(key) * max(eager, FLOOR)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- exact ----
def test_map_equals_the_dictionary():
    geo, pv = geometry(), pvmap()
    assert pv.n == 791 and pv.n_vox == [len(k) for k in geo.keys] == pv.tables.n
    for l in range(5):
        row = geo.row[l].cpu().numpy()
        assert np.array_equal(pv.row[l].cpu().numpy(), row)
        assert np.array_equal(pv.tables.coord[l].cpu().numpy(), np.array([k[1:] for k in geo.keys[l]]))
        assert np.array_equal(pv.counts(l).cpu().numpy(), np.bincount(row)) and int(pv.start[l][0]) == 0
        assert np.array_equal(pv.order[l].cpu().numpy(), np.argsort(row, kind="stable"))   # by voxel, ascending index within
        if l:
            assert torch.equal(pv.tables.parent[l - 1][pv.row[l - 1].long()], pv.row[l])


# ------------------------------------------------------------------------------------------ against float64 ----
def run_devox(level, C, fn, dtype):
    geo = geometry()
    rng = np.random.default_rng(100 * level + C)
    draw = lambda rows: torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).cuda().to(dtype)  # noqa: E731
    feat, add, g = draw(len(geo.keys[level])).requires_grad_(True), draw(geo.n).requires_grad_(True), draw(geo.n)
    out = fn(feat, level, add)
    g_feat, g_add = torch.autograd.grad(out, (feat, add), g)
    return {"out": out.detach(), "g_feat": g_feat, "g_add": g_add}


def run_vox(level, C, fn, dtype):
    geo = geometry()
    rng = np.random.default_rng(100 * level + C + 1)
    draw = lambda rows: torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).cuda().to(dtype)  # noqa: E731
    x, g = draw(geo.n).requires_grad_(True), draw(len(geo.keys[level]))
    v = fn(x, level)
    return {"v": v.detach(), "g_x": torch.autograd.grad(v, x, g)[0]}


def ours(kind, level, C):
    from ao_amd.spvcnn import devoxelize, voxelize

    if kind == "devox":
        return run_devox(level, C, lambda feat, l, add: devoxelize(feat, pvmap(), l, add=add), torch.float32)
    return run_vox(level, C, lambda x, l: voxelize(x, pvmap(), l), torch.float32)


@pytest.mark.parametrize("C", SC.DEVOX_C)
@pytest.mark.parametrize("level", SC.LEVELS_TESTED)
def test_devoxelize_against_float64(level, C):
    f64, f32 = (run_devox(level, C, lambda feat, l, add: R.devoxelize(feat, geometry(), l, add), dt) for dt in (torch.float64, torch.float32))
    check("devox-l%d-c%d" % (level, C), ours("devox", level, C), f64, f32, DEVOX_KEYS)


def test_devoxelize_at_level_0_is_the_gather():
    from ao_amd.spvcnn import devoxelize

    feat = torch.randn(pvmap().n_vox[0], 64, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    want = feat[pvmap().row[0].long()]
    assert ((devoxelize(feat, pvmap(), 0) - want).abs() <= 2e-8 * want.abs()).all()


@pytest.mark.parametrize("C", SC.VOX_C)
@pytest.mark.parametrize("level", SC.LEVELS_TESTED)
def test_voxelize_against_float64(level, C):
    f64, f32 = (run_vox(level, C, lambda x, l: R.voxelize(x, geometry(), l), dt) for dt in (torch.float64, torch.float32))
    check("vox-l%d-c%d" % (level, C), ours("vox", level, C), f64, f32, VOX_KEYS)


# ------------------------------------------------------------------------------------- repeatability, limits ----
@pytest.mark.parametrize("kind,C", [("devox", 96), ("vox", 6), ("vox", 256)])
def test_two_runs_give_the_same_bits(kind, C):
    a, b = ours(kind, 4, C), ours(kind, 4, C)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind,C", [("devox", 16), ("devox", 48), ("devox", 416), ("vox", 17), ("vox", 48), ("vox", 416)])
def test_an_unsupported_width_raises(kind, C):
    from ao_amd.spvcnn import devoxelize, voxelize

    with pytest.raises(ValueError):
        if kind == "devox":
            devoxelize(torch.zeros(pvmap().n_vox[2], C, device="cuda"), pvmap(), 2)
        else:
            voxelize(torch.zeros(791, C, device="cuda"), pvmap(), 2)
