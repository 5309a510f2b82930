"""GPU: the operators of ao_amd/msc/ops.py (ao_amd/csrc/msc.hip) against tests/msc_ref.py, on both paths (HIP and
AO_AMD_MSC=torch) where both exist.

Matching and masks are exact.  The InfoNCE loss follows the project's M-rule (DESIGN.md sections 2, 11, 13): the kernel's error
against float64 is at most M_TOL * max(the error of the reference's eager fp32 statements on the same GPU, 2^-24), relative
error for the three scalars and relative L2 for the two gradients.  At M = 1 and M = 2 alone a relative error is taken against
the larger of the value and the term that is subtracted in it -- the loss is mean(lse) - pos_sim / t, neg_sim is
mean(sim) - pos_sim / M, a gradient is that of the log-sum-exp plus that of the positive term -- because at M = 1 the two cancel
to an exact zero, of which no fp32 evaluation has a relative error.  M_TOL (tests/msc_cases.py): twice the worst ratio measured on an MI355X over the cases below, rounded up to a power
of two, at least 1 and at most 64; DESIGN.md section 13 lists the ratios."""
import numpy as np
import pytest
import torch

from tests import msc_ref as R
from tests.msc_cases import FLOOR, M_TOL, M_TOL_RUNNING_MAX, fixture

pytestmark = pytest.mark.gpu

SIZES = [(1, 96), (2, 96), (63, 96), (64, 96), (65, 96), (257, 96), (1000, 96), (257, 4), (257, 32), (257, 256)]
SPECIAL = ["dup2", "dup1", "zero_row", "scale_1e3", "scale_1e-3"]


def nce_case(name, m, c, seed):
    """(f1 (n1, c), f2 (n2, c), pairs (m, 2)): n1, n2 > m, so that some rows are named by no pair; matched rows are similar"""
    rng = np.random.default_rng(seed)
    n1, n2 = m + 37, m + 11
    pairs = np.stack([rng.permutation(n1)[:m], rng.permutation(n2)[:m]], 1).astype(np.int64)
    f1 = rng.normal(1.0, 1.0, (n1, c))
    f2 = rng.normal(1.0, 1.0, (n2, c))
    f2[pairs[:, 1]] = 0.6 * f1[pairs[:, 0]] + 0.4 * f2[pairs[:, 1]]
    if name == "dup2":  # one view-2 row taken by 50 pairs, and a few more repeats
        pairs[10:60, 1] = pairs[3, 1]
        pairs[100:104, 1] = pairs[99, 1]
    elif name == "dup1":
        pairs[20:27, 0] = pairs[5, 0]
        pairs[200:202, 0] = pairs[199, 0]
        pairs[30:33, 1] = pairs[29, 1]
    elif name == "zero_row":  # exercises the epsilon: a = 0 / (0 + 1e-7)
        f1[pairs[7, 0]] = 0.0
        f2[pairs[11, 1]] = 0.0
    elif name == "scale_1e3":
        f1, f2 = f1 * 1e3, f2 * 1e3
    elif name == "scale_1e-3":
        f1, f2 = f1 * 1e-3, f2 * 1e-3
    return f1.astype(np.float32), f2.astype(np.float32), pairs


def run_nce(f1, f2, pairs, t, g=1.7):
    from ao_amd import msc

    x1 = torch.from_numpy(f1).cuda().requires_grad_(True)
    x2 = torch.from_numpy(f2).cuda().requires_grad_(True)
    loss, pos_sim, neg_sim = msc.info_nce(x1, x2, torch.from_numpy(pairs).cuda(), t)
    assert not pos_sim.requires_grad and not neg_sim.requires_grad and loss.dtype == torch.float32
    (loss * g).backward()
    return dict(loss=loss.detach().cpu().numpy(), pos_sim=pos_sim.cpu().numpy(), neg_sim=neg_sim.cpu().numpy(),
                df1=x1.grad.cpu().numpy(), df2=x2.grad.cpu().numpy())


def errors(got, ref, t, m):
    """relative error (scalars) and relative L2 (gradients) against float64.  At M <= 2 the loss, neg_sim and the gradients are a
    difference of two terms that cancel (exactly at M = 1), and the error is taken against the larger of the value and the
    subtracted term; from M = 63 on against the value alone"""
    scale = dict.fromkeys(M_TOL, 0.0)
    if m <= 2:
        scale.update(loss=abs(ref["pos_sim"]) / t, neg_sim=abs(ref["pos_sim"]) / m, df1=np.linalg.norm(ref["df1_pos"]),
                     df2=np.linalg.norm(ref["df2_pos"]))
    return {k: float(np.linalg.norm(np.asarray(got[k], np.float64) - ref[k]) / max(np.linalg.norm(ref[k]), scale[k])) for k in M_TOL}


def check_nce(name, m, c, t, monkeypatch, tol=M_TOL):
    f1, f2, pairs = nce_case(name, m, c, seed=1000 + 7 * m + c)
    ref = R.info_nce(f1, f2, pairs, t, g=1.7)
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    got = run_nce(f1, f2, pairs, t)
    monkeypatch.setenv("AO_AMD_MSC", "torch")
    eager = run_nce(f1, f2, pairs, t)
    e_kernel, e_eager = errors(got, ref, t, m), errors(eager, ref, t, m)
    for k in M_TOL:
        print("msc info_nce %-10s M %4d C %3d t %.2f %-7s kernel %.3e eager %.3e ratio %.2f" % (
            name, m, c, t, k, e_kernel[k], e_eager[k], e_kernel[k] / max(e_eager[k], FLOOR)))
    for k in M_TOL:
        assert e_kernel[k] <= tol[k] * max(e_eager[k], FLOOR), (name, m, c, t, k, e_kernel[k], e_eager[k])
    # rows that no pair names: exactly zero
    unnamed1 = np.setdiff1d(np.arange(len(f1)), pairs[:, 0])
    unnamed2 = np.setdiff1d(np.arange(len(f2)), pairs[:, 1])
    assert len(unnamed1) >= 37 and len(unnamed2) >= 11
    assert not got["df1"][unnamed1].any() and not got["df2"][unnamed2].any()
    assert np.isfinite(got["df1"]).all() and np.isfinite(got["df2"]).all()


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("m,c", SIZES)
def test_info_nce_sizes(m, c, t, monkeypatch):
    check_nce("plain", m, c, t, monkeypatch)


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("name", SPECIAL)
def test_info_nce_special_rows(name, t, monkeypatch):
    check_nce(name, 257, 96, t, monkeypatch)


def test_info_nce_running_max_form(monkeypatch):
    """a temperature whose 2 / t leaves fp32's exp range takes the running-max form of the kernel"""
    check_nce("plain", 257, 96, 0.02, monkeypatch, tol=M_TOL_RUNNING_MAX)


def test_info_nce_same_bits_twice(monkeypatch):
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    for name, m, t in (("dup2", 257, 0.4), ("dup1", 257, 0.07), ("plain", 1000, 0.02)):
        f1, f2, pairs = nce_case(name, m, 96, seed=5)
        first, again = run_nce(f1, f2, pairs, t), run_nce(f1, f2, pairs, t)
        for k in first:
            assert np.array_equal(first[k], again[k]), (name, k)


def test_info_nce_outside_the_limits(monkeypatch):
    """C = 6 is no multiple of 4: the eager statements run, whatever the switch says; no pair at all raises"""
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    f1, f2, pairs = nce_case("plain", 65, 6, seed=9)
    got = run_nce(f1, f2, pairs, 0.4)
    x1, x2 = torch.from_numpy(f1).cuda().requires_grad_(True), torch.from_numpy(f2).cuda().requires_grad_(True)
    loss, pos_sim, neg_sim = msc.info_nce_torch(x1, x2, torch.from_numpy(pairs).cuda(), 0.4)
    (loss * 1.7).backward()
    assert np.array_equal(got["loss"], loss.detach().cpu().numpy()) and np.array_equal(got["df1"], x1.grad.cpu().numpy())
    assert np.array_equal(got["pos_sim"], pos_sim.cpu().numpy()) and np.array_equal(got["neg_sim"], neg_sim.cpu().numpy())
    assert np.array_equal(got["df2"], x2.grad.cpu().numpy())
    with pytest.raises(ValueError, match="no pair"):
        msc.info_nce(x1, x2, torch.zeros((0, 2), dtype=torch.int64, device="cuda"), 0.4)
    f1, f2, pairs = nce_case("plain", 65, 96, seed=9)
    pairs[4, 1] = len(f2)  # one past the end
    # a pair outside its operand: nothing is read outside a buffer, nothing is read back; the three outputs are NaN
    x1 = torch.from_numpy(f1).cuda().requires_grad_(True)
    out = msc.info_nce(x1, torch.from_numpy(f2).cuda(), torch.from_numpy(pairs).cuda(), 0.4)
    assert all(bool(torch.isnan(v)) for v in out)
    out[0].backward()
    assert bool(torch.isfinite(x1.grad).all()), "the backward reads nothing outside either"


def test_info_nce_under_autocast(monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    f1, f2, pairs = nce_case("plain", 65, 32, seed=3)
    want = run_nce(f1, f2, pairs, 0.4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, _, _ = msc.info_nce(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda(), torch.from_numpy(pairs).cuda(), 0.4)
    assert loss.dtype == torch.float32 and np.array_equal(loss.cpu().numpy(), want["loss"])


def test_no_m_by_m_tensor(monkeypatch):
    """M = 4096, C = 96, forward and backward: the allocator's peak rises by less than a quarter of one fp32 `sim` (16 MB; the
    kernels need about ten (M, C) arrays), where the eager statements need several whole ones.  A condition, not a measurement."""
    from ao_amd import msc

    m, c = 4096, 96
    f1, f2, pairs = nce_case("plain", m, c, seed=77)
    x1, x2 = torch.from_numpy(f1).cuda().requires_grad_(True), torch.from_numpy(f2).cuda().requires_grad_(True)
    index = torch.from_numpy(pairs).cuda()

    def rise(path):
        monkeypatch.setenv("AO_AMD_MSC", path)
        x1.grad = x2.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, _, _ = msc.info_nce(x1, x2, index, 0.4)
        loss.backward()
        torch.cuda.synchronize()
        assert x1.grad is not None and bool(torch.isfinite(loss))
        return torch.cuda.max_memory_allocated() - before

    hip, eager = rise("hip"), rise("torch")
    print("msc info_nce M 4096 C 96: allocator peak rises by %.1f MB (HIP), %.1f MB (eager)" % (hip / 2 ** 20, eager / 2 ** 20))
    assert hip < m * m * 4 // 4
    assert eager > 64 << 20


# ---------------------------------------------------------------------------------------------------------- matching ----
def random_views(seed, sizes, shift=None, box=1.0):
    """view 1 and view 2 of len(sizes) scenes: (n, 3) fp32 and the scene ends"""
    rng = np.random.default_rng(seed)
    c1, c2 = [], []
    for s, (n1, n2) in enumerate(sizes):
        c1.append(rng.uniform(-box / 2, box / 2, (n1, 3)))
        c2.append(rng.uniform(-box / 2, box / 2, (n2, 3)) + (0.0 if shift is None else shift[s]))
    ends = lambda parts: np.cumsum([len(p) for p in parts]).astype(np.int32)  # noqa: E731
    return np.concatenate(c1).astype(np.float32), ends(c1), np.concatenate(c2).astype(np.float32), ends(c2)


def match_cases():
    fix = fixture()
    recorded = (fix["view1_origin_coord"], fix["view1_offset"], fix["view2_origin_coord"], fix["view2_offset"])
    idx, d2 = R.knn_bruteforce(int(fix["max_k"]), recorded[2], recorded[3], recorded[0], recorded[1])
    radius = float(fix["radius"])
    cases = {
        "recorded_a": (recorded, 8, radius, int(fix["a.max_pair"]), R.spread_draws(idx, d2, radius, fix["a.match_draws"]),
                       fix["a.pair_perm"], fix["a.match_index"]),
        "recorded_b": (recorded, 8, radius, 8192, R.spread_draws(idx, d2, radius, fix["b.match_draws"]), None, fix["b.match_index"]),
        # the second scene's view 2 lies 10 m away: no match there at all
        "no_match_scene": (random_views(1, [(150, 140), (130, 120)], shift=[0.0, 10.0]), 4, 0.12, 8192, None, None, None),
        # dense: rows with k hits; eight far view-1 points: rows with none
        "k_hits": (random_views(2, [(260, 400)]), 4, 0.16, 8192, None, None, None),
        "over_max_pair": (random_views(3, [(200, 210), (150, 160)]), 6, 0.15, 64, None, "draw", None),
        "k1": (random_views(4, [(180, 170)]), 1, 0.1, 8192, None, None, None),
        "none": (random_views(5, [(50, 40), (30, 60)], shift=[5.0, -5.0]), 3, 0.1, 8192, None, None, None),
    }
    far = cases["k_hits"][0][0]
    far[:8] += np.float32(7.0)
    # exactly representable: neighbours at 0.125 and 0.1875 are hits, the one at exactly 0.25 is not (the comparison is strict)
    exact1 = np.array([[0, 0, 0], [4, 4, 4]], np.float32)
    exact2 = np.array([[0.25, 0, 0], [0.125, 0, 0], [0, 0.1875, 0], [4, 4.25, 4], [9, 9, 9]], np.float32)
    cases["on_the_radius"] = ((exact1, np.array([2], np.int32), exact2, np.array([5], np.int32)), 3, 0.25, 8192, None, None, None)
    return cases


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", ["recorded_a", "recorded_b", "no_match_scene", "k_hits", "over_max_pair", "k1", "none", "on_the_radius"])
def test_match_pairs(name, path, monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    (c1, o1, c2, o2), k, radius, max_pair, draws, perm, recorded = match_cases()[name]
    idx, d2 = R.knn_bruteforce(k, c2, o2, c1, o1)
    d = np.sqrt(d2[idx >= 0].astype(np.float64))
    on = d == radius
    assert (np.abs(d[~on] - radius) / radius > 1e-4).all(), "every distance is on the radius exactly or keeps its margin"
    counts = R.hit_counts(idx, d2, radius)
    rng = np.random.default_rng(11)
    if draws is None:
        draws = rng.integers(0, max(int(counts.max()), 1), len(c1))
    want = R.match(idx, d2, radius, draws)
    p = len(want)
    if isinstance(perm, str):
        perm = rng.permutation(p)
    want = R.cut_pairs(want, max_pair, perm)
    if recorded is not None:
        assert np.array_equal(want, recorded)
    if name == "no_match_scene":
        assert p > 0 and (want[:, 0] < o1[0]).all() and not counts[o1[0]:].any()
    if name == "k_hits":
        assert {0, 1, k} <= set(counts.tolist())
    if name == "over_max_pair":
        assert p > max_pair == len(want)
    if name == "none":
        assert p == 0
    if name == "on_the_radius":
        assert counts.tolist() == [2, 0] and (d == radius).sum() == 2
    dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).cuda()  # noqa: E731
    got = msc.match_pairs(dev(c1), dev(o1), dev(c2), dev(o2), k, radius, max_pair, row_draws=dev(draws), perm=dev(perm))
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (len(want), 2)
    assert np.array_equal(got.cpu().numpy(), want), name


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_match_pairs_draws_its_own(path, monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    c1, o1, c2, o2 = random_views(3, [(200, 210), (150, 160)])
    idx, d2 = R.knn_bruteforce(6, c2, o2, c1, o1)
    hit = (idx >= 0) & (np.sqrt(d2) < np.float32(0.15))
    p = int(hit.any(1).sum())
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    gen = torch.Generator(device="cuda").manual_seed(5)
    seen = set()
    for max_pair in (64, 8192):
        got = msc.match_pairs(dev(c1), dev(o1), dev(c2), dev(o2), 6, 0.15, max_pair, generator=gen).cpu().numpy()
        assert len(got) == min(p, max_pair) and len(set(got[:, 0].tolist())) == len(got), "view-1 rows are unique"
        for i, j in got:
            assert j in idx[i][hit[i]], "every pair is a true hit"
        seen.add(got.tobytes())
    assert len(seen) == 2


# ------------------------------------------------------------------------------------------------------- cross masks ----
def mask_cases():
    fix = fixture()
    rng = np.random.default_rng(21)
    recorded = (fix["view1_origin_coord"], fix["view1_offset"], fix["view2_origin_coord"], fix["view2_offset"])
    # coordinates exactly on multiples of the grid (as fp32 sees them): the cell is decided by the IEEE division alone
    lattice = lambda n: (rng.integers(-9, 10, (n, 3)) * 0.1).astype(np.float32)  # noqa: E731
    on_grid = (lattice(300), np.array([160, 300], np.int32), lattice(280), np.array([120, 280], np.int32))
    # a room of 6 m next to a blob of 15 cm
    big, small = rng.uniform(-3, 3, (300, 3)), rng.uniform(-0.07, 0.08, (40, 3))
    extent = (np.concatenate([big[:150], small[:20]]).astype(np.float32), np.array([150, 170], np.int32),
              np.concatenate([big[150:], small[20:]]).astype(np.float32), np.array([150, 170], np.int32))
    one = (rng.uniform(0.01, 0.09, (30, 3)).astype(np.float32), np.array([30], np.int32),
           rng.uniform(0.01, 0.09, (20, 3)).astype(np.float32), np.array([20], np.int32))
    return dict(recorded=recorded, on_grid=on_grid, extent=extent, one_patch=one, alias=alias_case())


def alias_case():
    """x spans cells -1 .. 2, so nx = trunc(2) + 1 = 3: cell (-1, 1, 0) gets id -1 + 3 = 2, the id of cell (2, 0, 0).  Both views
    have points in both cells, and in a few more"""
    rng = np.random.default_rng(22)
    cells = np.array([[-1, 1, 0], [2, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 1, 1], [2, 1, 1]])
    def view(n):  # noqa: E306
        which = np.concatenate([np.arange(len(cells)), rng.integers(0, len(cells), n - len(cells))])
        return ((cells[which] + rng.uniform(0.1, 0.9, (n, 3))) * 0.1).astype(np.float32), which
    (o1, w1), (o2, w2) = view(60), view(50)
    return o1, np.array([60], np.int32), o2, np.array([50], np.int32), w1, w2


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("rate", [0.0, 0.4, 0.5])
@pytest.mark.parametrize("name", ["recorded", "on_grid", "extent", "one_patch"])
def test_cross_masks(name, rate, path, monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    o1, f1, o2, f2 = mask_cases()[name]
    dev = lambda a: torch.from_numpy(np.asarray(a)).cuda()  # noqa: E731
    ids = R.patch_ids(o1, f1, o2, f2, 0.1)
    assert np.array_equal(msc.patch_ids(dev(o1), dev(f1), dev(o2), dev(f2), 0.1).cpu().numpy(), ids)
    patch_num = len(np.unique(ids))
    fix = fixture()
    perms = [np.random.default_rng(31).permutation(patch_num)]
    if name == "recorded" and rate in (0.0, 0.4):
        perms.append(fix["a.mask_perm" if rate == 0.4 else "b.mask_perm"])
    for perm in perms:
        want1, want2 = R.cross_masks(o1, f1, o2, f2, 0.1, rate, perm)
        got1, got2 = msc.cross_masks(dev(o1), dev(f1), dev(o2), dev(f2), 0.1, rate, perm=dev(perm))
        assert got1.dtype == torch.bool and got1.shape == (len(o1),) and got2.shape == (len(o2),)
        got1, got2 = got1.cpu().numpy(), got2.cpu().numpy()
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
        # no patch holds a mask-1 and a mask-2 point; of the m patches tagged for a view, exactly those that hold a point of
        # that view are masked in it, and every one of their points is
        m = int(patch_num * rate)
        p1, p2 = set(ids[:len(o1)][got1].tolist()), set(ids[len(o1):][got2].tolist())
        assert not p1 & p2
        _, cluster = np.unique(ids, return_inverse=True)
        c1, c2 = cluster.reshape(-1)[:len(o1)], cluster.reshape(-1)[len(o1):]
        tag1, tag2 = set(perm[:m].tolist()), set(perm[m:2 * m].tolist())
        assert set(c1[got1].tolist()) == tag1 & set(c1.tolist()) and set(c2[got2].tolist()) == tag2 & set(c2.tolist())
        assert not set(c1[~got1].tolist()) & tag1 and not set(c2[~got2].tolist()) & tag2
        if name in ("recorded", "extent") and rate > 0:  # (every patch of these holds points of both views, or nearly: count)
            assert 0 < len(set(c1[got1].tolist())) <= m and 0 < len(set(c2[got2].tolist())) <= m
        if name == "one_patch" or rate == 0.0:
            assert patch_num >= 1 and not got1.any() and not got2.any()
    if name == "recorded" and rate == 0.4:
        assert np.array_equal(got1, fix["a.mask1"]) and np.array_equal(got2, fix["a.mask2"])
    if name == "one_patch":
        assert patch_num == 1
    if name == "extent":
        assert patch_num > 100


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_cross_masks_keep_the_reference_aliasing(path, monkeypatch):
    """a negative cell shares its id, and so its mask, with another cell -- for every permutation; a partition that keeps the
    two apart separates them for some"""
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    o1, f1, o2, f2, w1, w2 = alias_case()
    dev = lambda a: torch.from_numpy(np.asarray(a)).cuda()  # noqa: E731
    ids = R.patch_ids(o1, f1, o2, f2, 0.1)
    assert set(ids[:60][w1 == 0].tolist()) == set(ids[:60][w1 == 1].tolist()) == {2}
    clean = R.alias_free_ids(o1, f1, o2, f2, 0.1)
    patch_num = len(np.unique(ids))
    assert len(np.unique(clean)) == patch_num + 1 == 9
    separated = 0
    for seed in range(20):
        perm = np.random.default_rng(seed).permutation(patch_num)
        got1, got2 = (m.cpu().numpy() for m in msc.cross_masks(dev(o1), dev(f1), dev(o2), dev(f2), 0.1, 0.5, perm=dev(perm)))
        assert len(set(got1[(w1 == 0) | (w1 == 1)].tolist())) == 1 and len(set(got2[(w2 == 0) | (w2 == 1)].tolist())) == 1
        want1, want2 = R.cross_masks(o1, f1, o2, f2, 0.1, 0.5, perm)
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
        clean1, clean2 = R.masks_of_ids(clean, 60, 0.5, np.random.default_rng(seed).permutation(patch_num + 1))
        separated += len(set(clean1[(w1 == 0) | (w1 == 1)].tolist())) == 2 or len(set(clean2[(w2 == 0) | (w2 == 1)].tolist())) == 2
    assert separated > 0


def test_cross_masks_draws_its_own(monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    o1, f1, o2, f2 = mask_cases()["extent"]
    dev = lambda a: torch.from_numpy(np.asarray(a)).cuda()  # noqa: E731
    gen = torch.Generator().manual_seed(2)
    a1, a2 = msc.cross_masks(dev(o1), dev(f1), dev(o2), dev(f2), 0.1, 0.4, generator=gen)
    b1, b2 = msc.cross_masks(dev(o1), dev(f1), dev(o2), dev(f2), 0.1, 0.4, generator=gen)
    assert bool(a1.any()) and bool(a2.any()) and not (torch.equal(a1, b1) and torch.equal(a2, b2))
    with pytest.raises(ValueError, match="mask_rate"):
        msc.cross_masks(dev(o1), dev(f1), dev(o2), dev(f2), 0.1, 0.51)


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("grid", [0.07, 0.3, 0.1])
def test_patch_ids_divide_in_ieee_fp32(grid, path, monkeypatch):
    """coordinates on and next to multiples of a grid whose fp32 reciprocal is inexact (1 / 0.07, 1 / 0.3): x / grid and
    x * (1 / grid) then fall into different cells for some of them, and both paths must take the division's"""
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", path)
    g = np.float32(grid)
    k = np.arange(-40, 41, dtype=np.float32)
    on = (k * g).astype(np.float32)
    line = np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))])
    by_division = np.floor(line / g)
    by_reciprocal = np.floor(line * (np.float32(1.0) / g))
    assert (by_division != by_reciprocal).any(), "the case tells the two apart"
    rng = np.random.default_rng(41)
    o1 = np.stack([line, rng.permutation(line), rng.permutation(line)], 1).astype(np.float32)
    o2 = np.stack([rng.permutation(line), line, rng.permutation(line)], 1).astype(np.float32)
    f1, f2 = np.array([100, len(o1)], np.int32), np.array([120, len(o2)], np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    got = msc.patch_ids(dev(o1), dev(f1), dev(o2), dev(f2), grid).cpu().numpy()
    assert np.array_equal(got, R.patch_ids(o1, f1, o2, f2, grid))


def test_patch_ids_refusals():
    from ao_amd import msc

    o, f = torch.zeros(8, 3, device="cuda"), torch.tensor([8], dtype=torch.int32, device="cuda")
    for args in ((o[:, :2], f, o, f, 0.1), (o, f, o, torch.tensor([4, 8], dtype=torch.int32, device="cuda"), 0.1), (o, f, o, f, 0.0),
                 (o[:0], f, o[:0], f, 0.1), (o, f[:0], o, f[:0], 0.1)):
        with pytest.raises(ValueError, match="patch ids"):
            msc.patch_ids(*args)
    with pytest.raises(RuntimeError, match="GPU only"):
        msc.patch_ids(o.cpu(), f, o, f, 0.1)
