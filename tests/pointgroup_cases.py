"""Seeded inputs of the PointGroup tests (tests/test_pointgroup_host.py, tests/test_gpu_pointgroup*.py, the fixture generator
tests/golden/make_golden_pointgroup.py).  Every case is built from a fixed seed and asserts its own preconditions on the CPU."""
import functools

import numpy as np

from tests import pointgroup_ref as R

MARGIN = 1e-4  # no pair of a case lies within MARGIN * r^2 of r^2 (unless it lies on it exactly, in exact arithmetic)
CAP = R.BALL_CAP


def _offsets(*counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _with_margin(draw, coords, offsets, radius, rng):
    """re-draws (from the same generator) the later point of every pair inside the margin until none is left"""
    r2 = float(radius) ** 2
    for _ in range(200):
        bad = set()
        for s in range(len(offsets) - 1):
            lo, hi = int(offsets[s]), int(offsets[s + 1])
            if hi > lo:
                i, j = np.nonzero(np.abs(R.pair_d2(coords, lo, hi) - r2) <= 2 * MARGIN * r2)
                bad.update((np.maximum(i, j) + lo).tolist())
        if not bad:
            break
        for p in sorted(bad):
            coords[p] = draw(rng)
    assert R.margin(coords, offsets, radius) > MARGIN
    return coords


@functools.lru_cache(maxsize=None)
def ball_cases():
    """{name: (coords (n, 3) fp32, batch_offsets (B + 1) int32, radius)}"""
    cases = {}
    # d2 = 4 is excluded and d2 = 3 included, exactly in any rounding
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    cases["lattice_strict"] = (g, _offsets(216), 2.0)
    rng = np.random.default_rng(1)
    draw = lambda r: r.uniform(0.0, 1.0, 3).astype(np.float32)  # noqa: E731
    one = _with_margin(draw, rng.uniform(0.0, 1.0, (150, 3)).astype(np.float32), _offsets(150), 0.3, rng)
    cases["two_clouds"] = (np.concatenate([one, one]), _offsets(150, 150), 0.3)  # no neighbour across the segments
    rng = np.random.default_rng(2)
    pts = rng.uniform(0.0, 1.0, (200, 3)).astype(np.float32)
    cases["empty_segment"] = (_with_margin(draw, pts, _offsets(80, 0, 120), 0.25, rng), _offsets(80, 0, 120), 0.25)
    cases["single"] = (np.array([[0.3, -2.0, 7.0]], np.float32), _offsets(1), 0.5)
    # negative coordinates, points on exact multiples of the radius: a 7^3 lattice of step 0.5 around the origin, radius 1;
    # d2 = 0.25 m exactly, m <= 3 is inside and m = 4 (a distance of exactly one radius) outside
    g = (np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.5).astype(np.float32)
    cases["cell_edges"] = (g[np.random.default_rng(3).permutation(g.shape[0])], _offsets(343), 1.0)
    rng = np.random.default_rng(4)
    pts = _with_margin(draw, rng.uniform(0.0, 1.0, (500, 3)).astype(np.float32), _offsets(500), 0.15, rng)
    pts = np.insert(pts, 250, np.float32(1e6), axis=0)  # one outlier: it must not size the cell table
    cases["outlier"] = (pts, _offsets(501), 0.15)
    rng = np.random.default_rng(5)
    # two clouds of 1 500 points with about 20 neighbours each: 1500 * (4 / 3) pi r^3 = 20 in a unit box
    radius = float((20 / 1500 / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))
    off = _offsets(1500, 1500)
    pts = _with_margin(draw, rng.uniform(0.0, 1.0, (3000, 3)).astype(np.float32), off, radius, rng)
    cases["random_margin"] = (pts, off, radius)
    for name, blob in (("cap", 1100), ("cap_exact", 1000), ("cap_1010", 1010)):
        cases[name] = cap_case(blob)[:3]
    for name, (coords, offsets, radius) in cases.items():
        assert coords.dtype == np.float32 and coords.shape == (int(offsets[-1]), 3), name
        m = R.margin(coords, offsets, radius)
        assert m > MARGIN or m == 0.0, (name, m)  # (0: a pair exactly on the radius, excluded in any rounding: the lattices)
    lists = R.ball_query(*cases["random_margin"])[0]
    assert 15 < np.mean([v.shape[0] for v in lists]) < 25
    # an interior point has the 27 points of its 3^3 cube (d2 <= 3); the 6 at d2 = 4 are outside
    assert max(v.shape[0] for v in R.ball_query(*cases["lattice_strict"])[0]) == 27
    return cases


def cap_case(blob):
    """`blob` coincident points whose indices are interleaved with 50 far points (one after every blob / 50 blob points):
    (coords, offsets, radius, is_blob)"""
    n = blob + 50
    step = n // 50
    is_blob = np.ones(n, bool)
    is_blob[step // 2::step] = False
    assert int((~is_blob).sum()) == 50 and int(is_blob.sum()) == blob
    coords = np.zeros((n, 3), np.float32)
    coords[~is_blob, 0] = 100.0 * (1 + np.arange(50))
    coords[is_blob] = (0.25, -0.5, 2.0)
    return coords, _offsets(n), 1.5, is_blob


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """{name: (coords, batch_offsets, radius, label (n) int32, min_points)}; the clusters follow from the ball query of the first
    three and tests/pointgroup_ref.py's search"""
    cases = {}
    # a chain of 200 points, spacing 1, radius 1.5, shuffled: a long diameter, the smallest index in the middle
    rng = np.random.default_rng(10)
    order = rng.permutation(200)
    order[order == 0], order[100] = order[100], 0
    assert order[100] == 0 and sorted(order) == list(range(200))
    coords = np.zeros((200, 3), np.float32)
    coords[order, 0] = np.arange(200)
    cases["chain"] = (coords, _offsets(200), 1.5, np.ones(200, np.int32), 50)
    # 7 rows of 20 points; the middle row carries another label and cuts the component in two
    g = np.stack(np.meshgrid(np.arange(7), np.arange(20), [0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    label = np.where(g[:, 0] == 3, 2, 1).astype(np.int32)
    perm = np.random.default_rng(11).permutation(140)
    cases["labels_touching"] = (g[perm], _offsets(140), 1.2, label[perm], 10)
    # chains of min_points - 1, min_points and min_points + 1 points, far apart
    sizes, coords = (9, 10, 11), []
    for c, size in enumerate(sizes):
        coords += [(i, 50.0 * c, 0.0) for i in range(size)]
    coords = np.array(coords, np.float32)
    perm = np.random.default_rng(12).permutation(coords.shape[0])
    cases["threshold"] = (coords[perm], _offsets(30), 1.5, np.ones(30, np.int32), 10)
    # four chains whose members alternate in index: point i belongs to chain i % 4
    coords = np.array([(i // 4, 30.0 * (i % 4), 0.0) for i in range(160)], np.float32)
    cases["interleaved"] = (coords, _offsets(160), 1.5, np.ones(160, np.int32), 5)
    coords, offsets, radius, _ = cap_case(1100)
    cases["capped_directed"] = (coords, offsets, radius, np.ones(coords.shape[0], np.int32), 50)
    cases["all_ignored"] = (np.zeros((0, 3), np.float32), _offsets(0), 1.5, np.zeros(0, np.int32), 50)
    return cases


def cluster_expected(name):
    """(idx, start_len, capped, rows, offsets, point_cluster) of a cluster case from tests/pointgroup_ref.py"""
    coords, offsets, radius, label, min_points = cluster_cases()[name]
    _, idx, start_len, capped = R.ball_query(coords, offsets, radius)
    rows, coffsets = R.bfs_cluster(label, idx, start_len, min_points)
    return idx, start_len, capped, rows, coffsets, R.point_cluster(rows, coords.shape[0])


def proposal_case():
    """clusters of 100, 101, 5 000 and 60 members among 9 000 points (three 4 096-point chunks), 7 classes:
    (point_cluster, sizes, firsts, rows, offsets, segment_pred, logits)"""
    rng = np.random.default_rng(20)
    n, sizes = 9000, (100, 101, 5000, 60)
    perm = rng.permutation(n)
    members, at = [], 0
    for size in sizes:
        members.append(np.sort(perm[at:at + size]))
        at += size
    members.sort(key=lambda m: m[0])  # clusters are numbered by their smallest member
    rows = np.concatenate([np.stack([np.full(m.shape[0], c), m], 1) for c, m in enumerate(members)]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([m.shape[0] for m in members])]).astype(np.int32)
    logits = rng.normal(0.0, 2.0, (n, 7)).astype(np.float32)
    segment_pred = R.softmax64(logits).argmax(1).astype(np.int64)
    sizes = np.array([m.shape[0] for m in members], np.int32)
    assert sorted(sizes.tolist()) == [60, 100, 101, 5000]
    return (R.point_cluster(rows, n), sizes, np.array([m[0] for m in members], np.int32), rows, offsets, segment_pred, logits)


def loss_case(n, seed, all_masked=False, special=True):
    """bias_pred, coord, instance_center (n, 3) fp32, instance (n) int64 with about 30 % of -1.  special: row 3 is used, has a
    zero bias_pred and a target of about 3e-15 (so that its gradient g * gt_norm / 1e-8 is of the size of the others'); in row 5,
    used, the first component of bias_pred equals its target exactly."""
    rng = np.random.default_rng(seed)
    coord = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    center = (coord + rng.normal(0.0, 0.5, (n, 3))).astype(np.float32)
    pred = rng.normal(0.0, 0.5, (n, 3)).astype(np.float32)
    instance = rng.integers(0, 12, n).astype(np.int64)
    instance[rng.uniform(size=n) < 0.3] = -1
    if special:
        instance[[3, 5]] = 1
        pred[3] = 0.0
        coord[3] = 0.0
        center[3] = (3e-15, -1e-15, 2e-15)
        coord[5, 0], center[5, 0], pred[5, 0] = 0.5, 0.75, 0.25
        assert np.float32(center[5, 0] - coord[5, 0]) == pred[5, 0] and float(center[5, 0]) - float(coord[5, 0]) == 0.25
    if all_masked:
        instance[:] = -1
    return pred, coord, center, instance


def kept_rows(grad64, instance, ignore=-1):
    """the used rows whose float64 gradient is not below 1e-6 of the largest: (mask of kept rows, their share of the used rows)"""
    used = instance != ignore
    size = np.abs(grad64).max(1)
    keep = used & (size >= 1e-6 * size.max())
    return keep, keep.sum() / max(used.sum(), 1)


PROPOSE_CFG = dict(semantic_num_classes=5, segment_ignore_index=(0,), cluster_thresh=1.5, cluster_propose_points=100,
                   cluster_min_points=50, voxel_size=0.02)


BLOBS = ((60, 1), (101, 2), (150, 3))  # (points, class)
CENTRES = np.array([(1.0, 1.0, 1.0), (2.0, 1.5, 0.5), (0.5, 2.5, 1.5), (2.5, 2.5, 2.5), (0.4, 0.6, 2.4)], np.float32)


def blob_scene(seed, blobs=BLOBS, ignored=40, clouds=2):
    """`clouds` clouds, each with the blobs (points whose coord + bias lies within about 0.3 voxels of a centre, the same
    centres in every cloud) and `ignored` points of class 0 that stay where they are, in shuffled order:
    dict(coord, offset, bias, logit, segment, instance, instance_center); instance numbers the blobs over the batch"""
    rng = np.random.default_rng(seed)
    coord, bias, logit, segment, instance, center = [], [], [], [], [], []
    for cloud in range(clouds):
        rows = [(c, cls) for c, (size, cls) in enumerate(blobs) for _ in range(size)] + [(-1, 0)] * ignored
        for c, cls in [rows[i] for i in rng.permutation(len(rows))]:
            xyz = rng.uniform(0.0, 3.0, 3)
            target = CENTRES[c] + rng.normal(0.0, 0.006, 3) if c >= 0 else xyz + rng.normal(0.0, 0.01, 3)
            z = rng.normal(0.0, 0.3, 5)
            z[cls] += 4.0
            coord.append(xyz), bias.append(target - xyz), logit.append(z), segment.append(cls)
            instance.append(cloud * len(blobs) + c if c >= 0 else -1)
            center.append(CENTRES[c] if c >= 0 else (-1.0, -1.0, -1.0))
    per_cloud = sum(size for size, _ in blobs) + ignored
    return dict(coord=np.array(coord, np.float32), offset=(per_cloud * (1 + np.arange(clouds))).astype(np.int32),
                bias=np.array(bias, np.float32), logit=np.array(logit, np.float32), segment=np.array(segment, np.int64),
                instance=np.array(instance, np.int64), instance_center=np.array(center, np.float32))


def scene_margin(scene, bias=None, logit=None):
    """(proposal sizes, ball-query margin) of a scene under PROPOSE_CFG, from tests/pointgroup_ref.py"""
    out = R.propose(scene["coord"], scene["offset"], scene["bias"] if bias is None else bias,
                    scene["logit"] if logit is None else logit, PROPOSE_CFG["segment_ignore_index"], PROPOSE_CFG["cluster_thresh"],
                    PROPOSE_CFG["cluster_min_points"], PROPOSE_CFG["cluster_propose_points"], PROPOSE_CFG["voxel_size"])
    return out[3], out[4]


@functools.lru_cache(maxsize=None)
def propose_case():
    """blobs of 60, 101 and 150 shifted points around three centres, the same centres in two clouds, and 40 points of the ignored
    class 0 per cloud: (coord, offset, bias_pred, logit_pred); the first seed whose shifted points keep the margin"""
    for seed in range(30, 130):
        scene = blob_scene(seed)
        sizes, margin = scene_margin(scene)
        if margin > MARGIN:
            break
    assert margin > MARGIN, "no seed keeps the ball query's margin"
    assert sorted(sizes.tolist()) == [101, 101, 150, 150], sizes
    return scene["coord"], scene["offset"], scene["bias"], scene["logit"]
