"""GPU: the PP2S label pipeline (ao_amd/ptv2/pp2s.py on ao_amd/csrc/pp2s.hip).

Everything but the alignment is integer or a choice, and the fixture's inputs are built so that the reference's choices do not
hang on a rounding (tests/golden/make_golden_pp2s.py asserts it: no projected coordinate within 1e-6 of a half-integer or a
bound, no |depth - z_cam| within 1e-6 of the tolerance, no p.z within 1e-6 of 0): every bridge, every visible count, seen_any,
the weak mask, the prompts of every view and the labels must EQUAL tests/golden/pp2s.npz (the reference's own statements) for
the two fixture rooms, and tests/pp2s_ref.py (pinned to that fixture on the CPU) for the small shapes.  The aligned room is
held to 2 * gamma_3 * sum |a_i| |b_i| per element (tests/pp2s_cases.align_bound): the reference's rotation is a BLAS product
whose order is not specified, both sides are within gamma_3 of the exact dot product.  Both paths run: HIP and AO_AMD_PP2S=torch.
"""
import warnings

import numpy as np
import pytest
import torch

from tests import pp2s_cases as PC
from tests import pp2s_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = ["hip", "torch"]
SIZES = [0, 1, 63, 64, 65, 257, 3001]


@pytest.fixture(scope="module")
def fx():
    return PC.load()


@pytest.fixture(scope="module")
def rooms(fx):
    """the fixture rooms and what the reference computed for them, built once"""
    return {tag: (case, PC.expected(fx, case)) for tag, case in ((t, PC.room(t)) for t in PC.CASES)}


def use(path, monkeypatch):
    if path == "torch":
        monkeypatch.setenv("AO_AMD_PP2S", "torch")
    else:
        monkeypatch.delenv("AO_AMD_PP2S", raising=False)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.cpu().numpy()


# ---- the two fixture rooms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tag", sorted(PC.CASES))
def test_fixture_stages(rooms, tag, path, monkeypatch):
    from ao_amd.ptv2 import LabelPropagator, align_room, bridge_to_numpy, choose_weak_labels, project_view

    use(path, monkeypatch)
    case, want = rooms[tag]
    n = case["n"]
    coord64 = align_room(dev(case["coord"]), case["angle"], case["center"])
    assert coord64.dtype == torch.float64 and coord64.shape == (n, 3)
    err = np.abs(host(coord64)[::PC.ALIGN_STRIDE] - want["aligned"])
    bound = PC.align_bound(case, slice(None, None, PC.ALIGN_STRIDE))
    print("aligned: max |device - fixture| = %.3e (bound: %.3e .. %.3e per element)" % (err.max(), bound.min(), bound.max()))
    assert (err <= bound).all()
    seen_any = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bridges = []
    for v, view in enumerate(case["views"]):
        bridge, count = project_view(coord64, view["k"], view["rt"], dev(view["depth"]), seen_any=seen_any)
        assert bridge.dtype == torch.int32 and bridge.shape == (n, 3) and count.is_cuda and count.dim() == 0
        assert np.array_equal(host(bridge), want["bridges"][v]) and int(count) == want["visible"][v]
        assert np.array_equal(bridge_to_numpy(bridge), want["bridges"][v].astype(np.uint16))
        bridges.append(bridge)
    # the same image as float64 with depth_scale=1
    again, count = project_view(coord64, case["views"][0]["k"], case["views"][0]["rt"],
                                dev(case["views"][0]["depth"] / PC.DEPTH_SCALE), depth_scale=1)
    assert torch.equal(again, bridges[0]) and int(count) == want["visible"][0]
    assert np.array_equal(host(seen_any), want["seen_any"])
    weak = choose_weak_labels(dev(case["instance"].reshape(-1)), seen_any)
    assert weak.dtype == torch.uint8 and np.array_equal(host(weak), want["weak"])
    prop = LabelPropagator(dev(case["semantic"]), weak, case["c"])
    for v, bridge in enumerate(bridges):
        idx, xy, cls = prop.view_prompts(bridge)
        assert idx.dtype == np.int64 and xy.dtype == np.int32 and cls.dtype == np.int32
        for got, ref in zip((idx, xy, cls), want["prompts"][v]):
            assert np.array_equal(got, ref)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tag", sorted(PC.CASES))
def test_fixture_scene(rooms, tag, path, monkeypatch):
    from ao_amd.ptv2 import pp2s_scene

    use(path, monkeypatch)
    case, want = rooms[tag]
    asked, d = [], {}

    def masks_for(key, xy, cls):
        asked.append(key)
        return dev(PC.masks_for(case, key, xy, cls))

    label = pp2s_scene(case["coord"], case["instance"], case["semantic"], PC.view_args(case), masks_for, case["c"], case["angle"],
                       case["center"], details=d)
    assert isinstance(label, np.ndarray) and label.shape == (case["n"], 1) and label.dtype == np.int32
    assert np.array_equal(label[:, 0], want["label"])
    keys = [v["key"] for v in case["views"]]
    assert [d["visible"][k] for k in keys] == want["visible"]
    assert sorted(d["bridges"]) == sorted(k for k, c in zip(keys, want["visible"]) if c)  # a view that sees nothing has no bridge
    assert asked == [k for k, p in zip(keys, want["prompts"]) if p[0].size]               # ... and one without a prompt no masks
    assert np.array_equal(host(d["weak"]), want["weak"]) and np.array_equal(host(d["seen_any"]), want["seen_any"])


# ---- the smallest shapes --------------------------------------------------------------------------------------------------------

def small_room(n, seed, size=(23, 17), views=3, c=13):
    """n points in a 5 x 4 x 2.8 m box, three cameras inside it, depth images rendered from the points themselves"""
    rng = np.random.default_rng(seed)
    center = np.array([2.5, -1.25, 1.5])
    coord = ((rng.random((n, 3)) - 0.5) * np.array([5.0, 4.0, 2.8]) + center).astype(np.float32)
    coord64 = PR.align(coord, 77, center)
    view_list = PC.make_views(rng, coord64, center, 5.0, 4.0, views, size)[:views - 1] if n else []
    if n:  # instead of the view that looks away: one through a lens so long that it sees a few pixels' worth of points
        view_list += PC.make_views(rng, coord64, center, 5.0, 4.0, 2, size, focal=400.0)[:1]
        view_list[-1]["key"] = "view9"
    instance = rng.integers(-3, 6, n).astype(np.int32) * 1000003
    semantic = rng.integers(-1, c, n).astype(np.int32)
    return dict(n=n, c=c, coord=coord, angle=77, center=center, instance=instance, semantic=semantic, views=view_list, size=size,
                seed=seed)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES)
def test_small_rooms(n, path, monkeypatch):
    from ao_amd.ptv2 import align_room, pp2s_scene

    use(path, monkeypatch)
    case = small_room(n, 100 + n)
    masks = lambda key, xy, cls: PC.masks_for(case, key, xy, cls)  # noqa: E731
    ref = PR.pp2s_scene(case["coord"], case["instance"], case["semantic"], PC.view_args(case), masks, case["c"], case["angle"],
                        case["center"])
    coord64 = host(align_room(dev(case["coord"]), case["angle"], case["center"]))
    assert coord64.shape == (n, 3) and (np.abs(coord64 - ref["coord64"]) <= PC.align_bound(case)).all()
    d = {}
    label = pp2s_scene(case["coord"], case["instance"], case["semantic"], PC.view_args(case), lambda *a: dev(masks(*a)), case["c"],
                       case["angle"], case["center"], details=d)
    assert label.shape == (n, 1) and np.array_equal(label, ref["label"])
    assert d["visible"] == ref["visible"] and sorted(d["bridges"]) == sorted(ref["bridges"])
    for key, bridge in ref["bridges"].items():
        assert np.array_equal(host(d["bridges"][key]), bridge)
        for got, want in zip(d["prompts"][key], ref["prompts"][key]):
            assert np.array_equal(got, want)
    assert np.array_equal(host(d["seen_any"]), ref["seen_any"]) and np.array_equal(host(d["weak"]), ref["weak"])
    if n >= 63:
        assert 0 < ref["seen_any"].sum() < n and (ref["label"] != -1).any()


# ---- projection -----------------------------------------------------------------------------------------------------------------

# K = [[8, 0, 4], [0, 8, 3], [0, 0, 1]], RT = [I | 0]: a point (X, Y, 2) lands on the pixel (4 X + 4, 4 Y + 3); the first
# coordinate is bounded by `height` = 2 * 4 - 1 = 7, the second by `width` = 2 * 3 - 1 = 5
K_SMALL, RT_SMALL = np.array([[8.0, 0, 4], [0, 8.0, 3], [0, 0, 1]]), np.eye(3, 4)


def at_pixel(x, y, z=2.0):
    return [(x - 4) * z / 8, (y - 3) * z / 8, z]


@pytest.mark.parametrize("path", PATHS)
def test_projection_edges(path, monkeypatch):
    from ao_amd.ptv2 import project_view

    use(path, monkeypatch)
    points = [at_pixel(1, 1), at_pixel(6, 4), at_pixel(7, 2), at_pixel(3, 5), at_pixel(0, 2), at_pixel(3, 0),  # 0-5
              at_pixel(2.5, 1.5), at_pixel(3.5, 2.5),        # 6, 7: ties go to the even pixel: (2, 2) and (4, 2)
              [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.25, -2.0],  # 8-10: 0 / 0, 1 / 0, behind the camera (pixel (3, 2))
              at_pixel(2, 3, 2.0625), at_pixel(2, 3, 2.25), at_pixel(5, 1, 1.9375), [np.nan, 0.0, 2.0]]  # 11-14: depth test
    coord64 = np.array(points, np.float64)
    depth = np.full((5, 7), 2.0)
    want = np.zeros((len(points), 3), np.int32)
    for i, row in {0: (1, 1), 1: (6, 4), 6: (2, 2), 7: (4, 2), 11: (2, 3), 13: (5, 1)}.items():
        want[i] = row + (1,)
    ref = PR.project(coord64, K_SMALL, RT_SMALL, depth, 0.1)
    assert np.array_equal(ref[0], want) and ref[1] == 6 and not ref[2]
    seen_any = torch.zeros(len(points), dtype=torch.uint8, device=DEV)
    seen_any[2] = 1  # a point an earlier view saw stays seen
    bridge, count = project_view(dev(coord64), K_SMALL, RT_SMALL, dev(depth), depth_scale=1, seen_any=seen_any)
    assert np.array_equal(host(bridge), want) and int(count) == 6
    assert host(seen_any).tolist() == [int(i == 2 or want[i, 2]) for i in range(len(points))]
    # the raw integer image: 1024 / 512 == 2.0
    bridge, count = project_view(dev(coord64), K_SMALL, RT_SMALL, dev(np.full((5, 7), 1024, np.int32)))
    assert np.array_equal(host(bridge), want) and int(count) == 6
    # a view that sees nothing: everything is occluded
    bridge, count = project_view(dev(coord64), K_SMALL, RT_SMALL, dev(np.full((5, 7), 0.5)), depth_scale=1)
    assert int(count) == 0 and not host(bridge).any()
    with pytest.raises(ValueError, match="uint16"):
        project_view(dev(coord64), np.array([[8.0, 0, 40000], [0, 8.0, 3], [0, 0, 1]]), RT_SMALL, dev(depth), depth_scale=1)


@pytest.mark.parametrize("path", PATHS)
def test_projection_outside_the_depth_image_is_skipped_and_reported(path, monkeypatch):
    from ao_amd.ptv2 import LabelPropagator, project_view
    from ao_amd.ptv2.pp2s import new_status, raise_for_status

    use(path, monkeypatch)
    rng = np.random.default_rng(9)
    pixels = [(int(x), int(y)) for x, y in zip(rng.integers(1, 7, 200), rng.integers(1, 5, 200))]
    coord64 = np.array([at_pixel(x, y) for x, y in pixels])
    depth = np.full((4, 6), 2.0)  # one row and one column short of the bounds: pixels with x == 6 or y == 4 are outside
    outside = np.array([x == 6 or y == 4 for x, y in pixels])
    assert 0 < outside.sum() < 200
    ref = PR.project(coord64, K_SMALL, RT_SMALL, depth, 0.1)
    assert ref[2] and ref[1] == (~outside).sum() and not ref[0][outside].any()
    status = new_status(DEV)
    bridge, count = project_view(dev(coord64), K_SMALL, RT_SMALL, dev(depth), depth_scale=1, status=status)
    assert np.array_equal(host(bridge), ref[0]) and int(count) == ref[1]  # the rest of the view is unaffected
    with pytest.raises(IndexError, match="pixel"):
        raise_for_status(status)
    prop = LabelPropagator(dev(np.zeros(200, np.int32)), dev(np.zeros(200, np.uint8)), 13, status)
    with pytest.raises(IndexError, match="pixel"):
        prop.finish()
    assert host(prop.finish(check=False)).tolist() == [-1] * 200
    torch.cuda.synchronize()
    # a second view on the same status words: the count is this view's own
    _, count = project_view(dev(coord64), K_SMALL, RT_SMALL, dev(np.full((5, 7), 2.0)), depth_scale=1, status=status)
    assert int(count) == 200


# ---- the weak choice ------------------------------------------------------------------------------------------------------------

def weak_cases():
    rng = np.random.default_rng(17)
    big = np.array([2 ** 31 - 1, -2 ** 31, -1, 0, 2 ** 31 - 2, -2 ** 31 + 1, 123456789, -987654321], np.int64)
    yield "one instance", np.full(257, 5), rng.random(257) < 0.3
    yield "one instance, unseen", np.full(65, -1), np.zeros(65, bool)
    yield "every point its own", rng.permutation(300) - 150, rng.random(300) < 0.5
    yield "extreme ids", big[rng.integers(0, big.size, 3001)], rng.random(3001) < 0.2
    inst = np.repeat(np.arange(6), 5) * 7 - 9
    seen = np.zeros(30, bool)
    seen[[1, 5, 8, 11, 12, 14, 29]] = True  # seen counts 1, 2, 3, 0, 0, 1: ranks 0, 1, 1, the middle, the middle, 0
    yield "seen counts", inst, seen
    for n in SIZES:
        yield "n = %d" % n, rng.integers(-4, 5, n) * 536870911, rng.random(n) < 0.4


@pytest.mark.parametrize("path", PATHS)
def test_weak_choice(path, monkeypatch):
    from ao_amd.ptv2 import choose_weak_labels

    use(path, monkeypatch)
    for name, inst, seen in weak_cases():
        inst, seen = inst.astype(np.int32), seen.astype(np.uint8)
        want = PR.weak_mask(inst, seen)
        a = choose_weak_labels(dev(inst), dev(seen))
        b = choose_weak_labels(dev(inst), dev(seen))
        assert np.array_equal(host(a), want), name
        assert torch.equal(a, b), name  # two runs, bit for bit
        assert want.sum() == np.unique(inst).size, name
        if name == "seen counts":
            assert np.nonzero(want)[0].tolist() == [1, 8, 12, 17, 22, 29]


# ---- votes ----------------------------------------------------------------------------------------------------------------------

def random_view(rng, n, height, width, prompts, c, bad_class=False):
    """a bridge that covers every pixel, the wrap rows (0, ., 1) and (., 0, 1) and invisible rows of junk; dense masks"""
    bridge = np.stack([rng.integers(0, width + 1, n), rng.integers(0, height + 1, n), (rng.random(n) < 0.8).astype(np.int64)], 1)
    bridge[bridge[:, 2] == 0, :2] = 10 ** 6
    if n > 8:
        bridge[3] = (0, 0, 1)
        bridge[4] = (width, height, 1)
        bridge[5] = (7, 7, 2)  # the reference's test is `== 1`: not visible
    cls = rng.integers(0, c, prompts)
    if prompts > 2:
        cls[0], cls[1] = c - 1, 0
    if bad_class and prompts:
        cls[prompts // 2] = c
    masks = rng.random((prompts, height, width)) < 1.2 / max(prompts, 1)
    if prompts > 2 and n > 8:  # element [1][1] belongs to the mask of the last class alone, and row 6 sits on it
        masks[:, 1, 1] = False
        masks[0, 1, 1] = True
        bridge[6] = (2, 2, 1)
    return bridge.astype(np.int32), masks, cls.astype(np.int32)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("height,width", [(5, 7), (6, 6), (8, 8), (47, 63)])  # h w odd; h w % 4 == 0 with w % 4 != 0; w % 4 == 0
@pytest.mark.parametrize("prompts", [0, 1, 33, 70])
def test_votes(prompts, height, width, path, monkeypatch):
    from ao_amd.ptv2 import LabelPropagator

    use(path, monkeypatch)
    for c, n in ((2, 65), (32, 257), (13, 3001)):
        rng = np.random.default_rng([prompts, height, width, c])
        gt = rng.integers(-1, c, n).astype(np.int32)
        weak = (rng.random(n) < 0.1).astype(np.uint8)
        weak[6] = 0
        prop = LabelPropagator(dev(gt), dev(weak), c)
        seen_bits = np.zeros(n, np.uint32)
        for view in range(3):
            bridge, masks, cls = random_view(rng, n, height, width, prompts, c)
            assert PR.vote_view(seen_bits, bridge, masks, cls, c) == (False, False)
            m = dev(masks) if view else dev(masks).to(torch.uint8) * 255  # bool and uint8, any non-zero byte
            if view == 2 and prompts:  # a view of a buffer that starts on an odd byte
                m = torch.cat([torch.zeros(1, dtype=torch.bool, device=DEV), m.reshape(-1)])[1:].reshape(masks.shape)
            assert prop.vote_view(dev(bridge), m, dev(cls)) == prompts
        assert np.array_equal(host(prop.seen_bits).view(np.uint32), seen_bits)
        assert np.array_equal(host(prop.finish()), PR.labels(seen_bits, weak, gt))
        if prompts > 2:
            assert seen_bits[6] == np.uint32(1) << np.uint32(c - 1) and int(prop.label[6]) == c - 1  # class 31 when c == 32


@pytest.mark.parametrize("path", PATHS)
def test_vote_semantics(path, monkeypatch):
    from ao_amd.ptv2 import LabelPropagator

    use(path, monkeypatch)
    height, width, c = 4, 6, 32
    #                 x  y  visible
    bridge = np.array([[2, 1, 1],   # 0: element [0][1]
                       [0, 0, 1],   # 1: wraps to the last row and column, [3][5]
                       [3, 2, 1],   # 2: [1][2]: two masks of the SAME class
                       [4, 3, 1],   # 3: [2][3]: a class in view A, another in view B
                       [5, 4, 1],   # 4: [3][4]: a weak point under a foreign mask
                       [6, 1, 1],   # 5: [0][5]: a weak point whose ground truth is -1
                       [1, 1, 1],   # 6: [0][0]: NOT cleared
                       [2, 2, 0],   # 7: not visible, although a mask holds its element
                       [1, 4, 1]],  # 8: [3][0]: no mask
                      np.int32)
    gt = np.array([3, 3, 3, 3, 9, -1, 31, 5, 5], np.int32)
    weak = np.array([0, 0, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    prop = LabelPropagator(dev(gt), dev(weak), c)
    idx, xy, cls = prop.view_prompts(dev(bridge))
    assert idx.tolist() == [4] and xy.tolist() == [[5, 4]] and cls.tolist() == [9]  # 5: gt -1, 7: not seen -- no prompts

    def view(elements, classes):
        masks = np.zeros((len(classes), height, width), bool)
        for p, cells in enumerate(elements):
            for r, q in cells:
                masks[p, r, q] = True
        return dev(masks), dev(np.array(classes, np.int32))

    prop.vote_view(dev(bridge), *view([[(0, 1), (1, 2), (2, 3)], [(1, 2), (3, 5)], [(3, 4), (0, 5), (0, 0), (1, 1)]], [3, 3, 31]))
    prop.vote_view(dev(bridge), *view([[(2, 3), (0, 1)]], [4]))
    label = host(prop.finish()).tolist()
    #                0: 3 then 4  1: wrap  2: twice 3  3: 3 then 4  4: gt wins  5: not written over  6: [0][0]  7: weak  8: none
    assert label == [-1, 3, 3, -1, 9, 31, 31, 5, -1]
    assert host(prop.seen_bits).view(np.uint32).tolist() == [(1 << 3) | (1 << 4), 1 << 3, 1 << 3, (1 << 3) | (1 << 4), 1 << 31,
                                                             1 << 31, 1 << 31, 0, 0]


@pytest.mark.parametrize("path", PATHS)
def test_bad_prompt_class_and_bad_pixel_are_skipped_and_reported(path, monkeypatch):
    from ao_amd.ptv2 import LabelPropagator

    use(path, monkeypatch)
    rng = np.random.default_rng(4)
    n, c, height, width = 300, 13, 6, 6
    gt, weak = rng.integers(0, c, n).astype(np.int32), np.zeros(n, np.uint8)
    bridge, masks, cls = random_view(rng, n, height, width, 33, c, bad_class=True)
    clean = LabelPropagator(dev(gt), dev(weak), c)
    clean.vote_view(dev(bridge), dev(np.delete(masks, 16, 0)), dev(np.delete(cls, 16)))
    prop = LabelPropagator(dev(gt), dev(weak), c)
    prop.vote_view(dev(bridge), dev(masks), dev(cls))
    with pytest.raises(IndexError, match="class"):
        prop.finish()
    torch.cuda.synchronize()
    assert torch.equal(prop.seen_bits, clean.seen_bits) and int((clean.seen_bits != 0).sum()) > 50  # as without that prompt
    clean.finish()
    # a visible row outside [0, width] x [0, height]
    for column, value in ((0, width + 1), (1, height + 1), (0, -1)):
        off = bridge.copy()
        victim = int(np.nonzero(off[:, 2] == 1)[0][7])
        off[victim, column] = value
        gone = bridge.copy()
        gone[victim, 2] = 0
        a, b = LabelPropagator(dev(gt), dev(weak), c), LabelPropagator(dev(gt), dev(weak), c)
        a.vote_view(dev(off), dev(masks[:16]), dev(cls[:16]))
        b.vote_view(dev(gone), dev(masks[:16]), dev(cls[:16]))
        with pytest.raises(IndexError, match="pixel"):
            a.finish()
        torch.cuda.synchronize()
        assert torch.equal(a.seen_bits, b.seen_bits)
    with pytest.raises(ValueError, match="masks"):
        prop.vote_view(dev(bridge), dev(masks[:5]), dev(cls))
    with pytest.raises(ValueError, match="classes"):
        LabelPropagator(dev(gt), dev(weak), 33)


# ---- streams and synchronisation --------------------------------------------------------------------------------------------------

def test_current_stream_and_host_reads(rooms, monkeypatch):
    """everything is enqueued on the current stream; project_view, choose_weak_labels, vote_view and finish(check=False) read
    nothing back, the LabelPropagator's constructor and view_prompts once each"""
    from ao_amd.ptv2 import LabelPropagator, align_room, choose_weak_labels, project_view

    use("hip", monkeypatch)
    case, want = rooms["c13"]
    n = case["n"]
    coord, instance, semantic = dev(case["coord"]), dev(case["instance"].reshape(-1)), dev(case["semantic"])
    depths = [dev(v["depth"] / PC.DEPTH_SCALE) for v in case["views"]]
    served = [(dev(PC.masks_for(case, v["key"], p[1], p[2])), dev(p[2])) for v, p in zip(case["views"], want["prompts"])]
    warm = align_room(coord, case["angle"], case["center"])  # warm: the workspace, the kernels
    seen = torch.zeros(n, dtype=torch.uint8, device=DEV)
    b, _ = project_view(warm, case["views"][0]["k"], case["views"][0]["rt"], depths[0], depth_scale=1, seen_any=seen)
    w = choose_weak_labels(instance, seen)
    LabelPropagator(semantic, w, case["c"]).vote_view(b, *served[0])
    torch.cuda.synchronize()

    def reads(fn):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return out, len([w for w in seen if "called a synchronizing" in str(w.message)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        coord64, count = reads(lambda: align_room(coord, case["angle"], case["center"]))
        assert count == 0
        seen_any = torch.zeros(n, dtype=torch.uint8, device=DEV)
        bridges = []
        for view, depth in zip(case["views"], depths):
            (bridge, _), count = reads(lambda: project_view(coord64, view["k"], view["rt"], depth, depth_scale=1, seen_any=seen_any))
            assert count == 0
            bridges.append(bridge)
        weak, count = reads(lambda: choose_weak_labels(instance, seen_any))
        assert count == 0
        prop, count = reads(lambda: LabelPropagator(semantic, weak, case["c"]))
        assert count == 1
        for v, bridge in enumerate(bridges):
            (idx, _, _), count = reads(lambda: prop.view_prompts(bridge))
            assert count == 1 and np.array_equal(idx, want["prompts"][v][0])
            _, count = reads(lambda: prop.vote_view(bridge, *served[v]))
            assert count == 0
        label, count = reads(lambda: prop.finish(check=False))
        assert count == 0 and label.is_cuda
    side.synchronize()
    assert np.array_equal(host(weak), want["weak"]) and np.array_equal(host(label), want["label"])


# ---- the bridge goes into REAL's refinement as it is ------------------------------------------------------------------------------

def test_bridge_feeds_the_label_refiner(monkeypatch):
    from ao_amd.ptv2 import LabelRefiner, project_view
    from tests import refine_cases as RC

    use("hip", monkeypatch)
    case = RC.make_room("chain", 5, 300, 13, 3.2, 2.7, flat=(2.0, 9.5, 12.0))
    coord64 = case["coord"].astype(np.float64)
    size = (24, 16)
    k = np.array([[14.0, 0, 12.5], [0, 14.0, 8.5], [0, 0, 1]])
    rt = PC.look_at((2.6, -4.0, 1.5), (2.6, 1.35, 1.5))
    bridge, count = project_view(dev(coord64), k, rt, dev(PC.render_depth(coord64, k, rt, size)))
    assert bridge.dtype == torch.int32 and bridge.is_contiguous() and bridge.shape == (300, 3) and int(count) > 50
    r = LabelRefiner(13).begin(dev(case["logits"]), dev(case["coord"]), dev(case["label"].reshape(-1), torch.int32), dev(case["present"]))
    idx = host(r.prompt_idx)
    sees = int((host(bridge)[idx, 2] == 1).sum())
    assert idx.size > 0 and sees > 0
    # REAL indexes mask[u - 1][v - 1] with (u, v) = bridge[:, :2]: its masks are (P, x extent, y extent)
    assert r.vote_view(bridge, lambda xy, cls: torch.ones((len(cls), size[0], size[1]), dtype=torch.bool, device=DEV)) == sees
    label, updated, touched = r.finish()
    assert touched and label.shape == (300,)
