"""The scenes of the instance-evaluator tests (ao_amd/pointgroup/evaluate.py): seeded, 4 000 points each,
written as ranges of a layout that a seeded permutation then scatters over the point order.  Each scene asserts the cases it was
written to carry; tests/golden/make_golden_inseval.py runs the reference's evaluator on them and tests/golden/inseval.npz holds
what it returned.

    class 0   ignored, like -1            class 4   ground truth, never predicted (AP 0)
    class 1   the main class              class 5   neither (NaN)
    class 2   a second class              class 6   scene "ignored": ground truth, every prediction ignored (empty y_score)
    class 3   predicted, never in gt (NaN)
"""
import numpy as np

N = 4000
NUM_CLASSES = 7
NAMES = ["c0", "c1", "c2", "c3", "c4", "c5", "c6"]
SEGMENT_IGNORE = (-1, 0)
INSTANCE_IGNORE = -1
MIN_REGION = 100
SCENES = ("a", "b", "random", "ignored")


def _build(seed, layout, proposals):
    """layout: (stop, segment, instance) ranges from 0; proposals: (class, score, value, [(start, stop), ...])"""
    segment, instance = np.empty(N, np.int64), np.empty(N, np.int64)
    start = 0
    for stop, seg, inst in layout:
        segment[start:stop], instance[start:stop] = seg, inst
        start = stop
    assert start == N
    masks = np.zeros((len(proposals), N), np.int32)
    for row, (_, _, value, ranges) in enumerate(proposals):
        for lo, hi in ranges:
            masks[row, lo:hi] = value
    perm = np.random.default_rng(seed).permutation(N)
    return dict(masks=np.ascontiguousarray(masks[:, perm]), scores=np.array([p[1] for p in proposals], np.float32),
                classes=np.array([p[0] for p in proposals], np.int64), segment=segment[perm], instance=instance[perm])


def _count(scene, row, **where):
    """set points of a proposal among the points with the given instance / segment"""
    sel = scene["masks"][row] != 0
    for key, value in where.items():
        sel = sel & np.isin(scene[key], value)
    return int(sel.sum())


def _iou(scene, row, inst):
    inter = _count(scene, row, instance=inst)
    return inter / (int((scene["instance"] == inst).sum()) + _count(scene, row) - inter)


def scene_a():
    layout = ((600, 1, 7), (1000, 1, 12), (1060, 1, 40), (1500, 2, 3), (1900, 4, 21), (2400, 1, -1), (3000, -1, -1),
              (3300, 0, 55), (4000, 2, 90))
    proposals = ((1, 0.9, 1, [(0, 560)]), (1, 0.8, 1, [(50, 600)]), (1, 0.7, 1, [(500, 700)]),
                 (1, 0.85, 1, [(600, 1000), (2400, 2500)]), (1, 0.6, 1, [(1000, 1060), (1900, 2000)]), (1, 0.97, 1, [(0, 80)]),
                 (0, 0.96, 1, [(3000, 3300)]), (2, 0.95, 2, [(1060, 1500)]), (2, 0.75, 1, [(3300, 3800)]),
                 (3, 0.5, 1, [(1900, 2300)]), (2, 0.4, -1, [(3800, 4000), (2500, 2700)]), (1, 0.75, 1, [(1900, 2150)]))
    s = _build(0, layout, proposals)
    assert sorted(np.unique(s["instance"]).tolist()) == [-1, 3, 7, 12, 21, 40, 55, 90], "non-contiguous ids"
    assert _iou(s, 0, 7) > 0.9 and _iou(s, 1, 7) > 0.9, "two proposals over one gt, both above 0.5 (and above 0.9)"
    assert _count(s, 2, instance=7) == 100 and _count(s, 2, instance=12) == 100, "a proposal straddling two gts of its class"
    assert _count(s, 3, segment=SEGMENT_IGNORE) == 100 and _iou(s, 3, 12) == 0.8, "void points inside a proposal"
    assert (s["instance"] == 40).sum() == 60 and _count(s, 4, instance=40) == 60 and _count(s, 4) == 160, \
        "a gt below 100 points overlapped by a proposal whose ignored share is 0.375: above 0.25, not above 0.5"
    assert _count(s, 5) == 80 and s["classes"][5] == 1, "a proposal below 100 points"
    assert s["classes"][6] == 0 and _count(s, 6) == 300, "a proposal of an ignored class"
    assert ((s["segment"] == 1) & (s["instance"] == -1)).sum() == 500, "a valid segment with instance -1"
    assert ((s["segment"] == 0) & (s["instance"] == 55)).sum() == 300, "void points that carry an instance id"
    assert set(np.unique(s["masks"]).tolist()) == {-1, 0, 1, 2}, "mask values other than 0 / 1"
    assert (s["segment"] == 4).any() and not (s["classes"] == 4).any(), "a class with gt and no prediction"
    assert (s["classes"] == 3).any() and not (s["segment"] == 3).any(), "a class predicted and never in gt"
    assert _count(s, 10, segment=SEGMENT_IGNORE) * 2 == _count(s, 10) and _iou(s, 10, 90) < 0.25, "an ignored share of exactly 0.5"
    return s


def scene_b():
    layout = ((800, 1, 100), (1500, 2, 5), (1590, 2, 6), (2600, -1, -1), (3400, 1, 2), (4000, 2, -1))
    proposals = ((1, 0.75, 1, [(0, 700)]), (1, 0.75, 1, [(2600, 3100)]), (1, 0.65, 1, [(3000, 3400)]),
                 (2, 0.9, 1, [(800, 1590)]), (2, 0.3, 1, [(1500, 1650)]), (3, 0.2, 1, [(3400, 3600)]), (2, 0.75, 1, [(3400, 4000)]),
                 (1, 0.98, 1, [(100, 190)]), (0, 0.5, 1, [(1590, 2000)]), (1, 0.55, 7, [(0, 800), (2600, 3400)]),
                 (2, 0.6, 1, [(900, 1400)]), (1, 0.99, 1, [(2600, 3400)]))
    s = _build(1, layout, proposals)
    assert float(s["scores"][0]) == float(scene_a()["scores"][8]) == 0.75, "tied scores across scenes (and classes)"
    assert _iou(s, 2, 2) == 0.5 and _iou(s, 9, 2) == 0.5 and _iou(s, 9, 100) == 0.5, "an overlap of exactly 0.5 is not above 0.5"
    assert _count(s, 4, instance=6) == 90 and _count(s, 4, segment=SEGMENT_IGNORE) == 60, "a proposal that is ignored at every overlap"
    assert _count(s, 7) == 90 and s["classes"][8] == 0
    assert not (s["segment"] == 5).any() and not (s["classes"] == 5).any(), "a class with neither"
    return s


def scene_random():
    rng = np.random.default_rng(2)
    cuts = np.sort(rng.choice(np.arange(100, 3900), 9, replace=False)).tolist() + [N]
    ids = rng.choice(1000, len(cuts), replace=False)
    layout = []
    for stop, inst in zip(cuts, ids):
        seg = int(rng.choice([1, 2, -1, 1, 2]))
        layout.append((stop, seg, int(inst) if seg >= 0 and rng.uniform() < 0.85 else -1))
    proposals = []
    for _ in range(12):
        lo = int(rng.integers(0, 3800))
        hi = min(N, lo + int(rng.integers(50, 900)))
        proposals.append((int(rng.choice([1, 2, 1, 2, 3, 0])), round(float(rng.uniform()), 1), int(rng.choice([1, 1, 3, -2])), [(lo, hi)]))
    s = _build(2, tuple(layout), tuple(proposals))
    assert len(np.unique(s["scores"])) < 12, "rounded scores tie"
    return s


def scene_ignored():
    layout = ((300, 6, 1), (1000, -1, -1), (2000, 1, 4), (4000, 2, -1))
    proposals = ((6, 0.8, 1, [(300, 500)]), (6, 0.7, 1, [(500, 700), (0, 10)]), (1, 0.75, 1, [(1000, 1900)]), (2, 0.5, 1, [(2000, 2500)]))
    s = _build(3, layout, proposals)
    assert (s["instance"] == 1).sum() == 300 and _count(s, 0, segment=SEGMENT_IGNORE) == 200, "gt exists; a prediction wholly void"
    assert _count(s, 1, segment=SEGMENT_IGNORE) / _count(s, 1) > 0.9 and 0 < _iou(s, 1, 1) < 0.25, "ignored above every overlap"
    return s


def scenes():
    """{name: dict(masks (P, N) int32, scores (P) fp32, classes (P) int64, segment (N) int64, instance (N) int64)}"""
    return dict(a=scene_a(), b=scene_b(), random=scene_random(), ignored=scene_ignored())


def origin_case():
    """scene a seen from 6 000 origin points: a seeded nn_idx into its 4 000 points, with labels of their own"""
    s = scene_a()
    rng = np.random.default_rng(7)
    nn_idx = rng.integers(0, N, 6000).astype(np.int32)
    segment, instance = s["segment"][nn_idx].copy(), s["instance"][nn_idx].copy()
    flip = rng.uniform(size=6000) < 0.05  # the origin labels are not the sampled ones everywhere
    segment[flip], instance[flip] = -1, -1
    return s, nn_idx, segment, instance


RECORD_KEYS = ("gt_instance_id", "gt_segment_id", "gt_vert_count", "pred_row", "pred_class", "pred_conf", "pred_vert_count",
               "pred_void", "inter")
