"""Seeded synthetic rooms, views, depth images and masks shared by tests/golden/make_golden_pp2s.py,
tests/test_pp2s_host.py, tests/test_gpu_pp2s.py and tools/bench_pp2s.py (no test in here).  Everything is built on the CPU with
numpy from a seed; the fixture (tests/golden/pp2s.npz) stores the reference's OUTPUTS for these inputs and a digest of the
inputs, which `load()` compares, so that a numpy whose generators drew other numbers fails loudly instead of comparing
against the wrong room.

A room: points uniform in a box, turned away from the axes by the room's angle (the alignment turns it back); an instance
per 1.5 m patch of the floor plan and a class per instance.  Special instances: id -1, a single point, one with exactly two
seen points, one that no view sees, one whose ground truth is -1.  A view is a pinhole camera on a NON-square image (63 x 47:
K[0][2] != K[1][2], so a swapped axis fails); its depth image is rendered from the room's own points (the nearest per pixel,
quantised to 1 / 512 as the PNGs are) plus an occluder, so that a view has visible, occluded and out-of-frame points.  The
last but one view sees points but no weak point; the last one looks away from the room and sees nothing.
"""
import hashlib
import os

import numpy as np

from tests import pp2s_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEPTH_SCALE, TOL, FAR = 512.0, 0.1, 60.0
ALIGN_STRIDE = 8  # the fixture keeps every 8th row of the aligned room

#        tag: (seed, points, classes, box x, box y, angle, centre, views, image (x, y))
CASES = {"c13": (31, 3000, 13, 6.3, 4.6, 33, (3.6125, 2.2875, 1.4375), 5, (63, 47)),
         "c20": (47, 4000, 20, 5.2, 5.9, 270, (-2.9875, 7.1625, 1.3125), 4, (55, 41))}


def room(tag):
    return make_room(tag, *CASES[tag])


def look_at(eye, target):
    """RT (3, 4) of a camera at `eye` looking at `target`: x right, y down, z forward"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    rot = np.stack([right, down, fwd])
    return np.concatenate([rot, -(rot @ eye)[:, None]], 1)


def render_depth(coord64, k_matrix, rt_matrix, size, rng=None):
    """(H, W) raw integer depth: the nearest point in front of the camera per pixel, FAR where none; an occluding rectangle"""
    width, height = size
    krt = np.matmul(k_matrix, rt_matrix)
    pz = PR.row_dot(krt, 2, coord64)
    z_cam = PR.row_dot(rt_matrix, 2, coord64)
    front = z_cam > 0.2
    rx = np.round(PR.row_dot(krt, 0, coord64)[front] / pz[front]).astype(np.int64)
    ry = np.round(PR.row_dot(krt, 1, coord64)[front] / pz[front]).astype(np.int64)
    ok = (rx >= 0) & (rx < width) & (ry >= 0) & (ry < height)
    depth = np.full((height, width), FAR)
    np.minimum.at(depth, (ry[ok], rx[ok]), z_cam[front][ok])
    if rng is not None:
        x0, y0 = rng.integers(4, width // 2), rng.integers(4, height // 2)
        depth[y0:y0 + height // 3, x0:x0 + width // 4] = 0.31
    return np.round(depth * DEPTH_SCALE).astype(np.int32)


def make_views(rng, coord64, center, box_x, box_y, views, size, focal=None):
    center = np.asarray(center, np.float64)
    k_matrix = np.array([[focal or 0.8 * size[0], 0.0, (size[0] + 1) / 2], [0.0, focal or 0.8 * size[0], (size[1] + 1) / 2],
                         [0.0, 0.0, 1.0]])
    out = []
    for v in range(views):
        turn = 2 * np.pi * v / max(views - 1, 1) + 0.4
        eye = center + np.array([0.42 * box_x * np.cos(turn), 0.42 * box_y * np.sin(turn), 0.3 + 0.1 * v])
        target = center + np.array([-0.2 * box_x * np.cos(turn), -0.25 * box_y * np.sin(turn), -0.5])
        if v == views - 1:  # outside the room, looking away from it: every point is behind the camera
            eye = center + np.array([box_x, 0.0, 0.0])
            target = eye + np.array([1.0, 0.1, 0.0])
        rt_matrix = look_at(eye, target)
        out.append(dict(key="view%d" % v, k=k_matrix, rt=rt_matrix, depth=render_depth(coord64, k_matrix, rt_matrix, size, rng)))
    return out


def bridges_of(coord64, views):
    """[(bridge, count)] per view and seen_any, by the restatement"""
    seen_any = np.zeros(coord64.shape[0], np.uint8)
    out = []
    for view in views:
        bridge, count, skipped = PR.project(coord64, view["k"], view["rt"], view["depth"] / DEPTH_SCALE, TOL)
        assert not skipped
        out.append((bridge, count))
        seen_any[bridge[:, 2] == 1] = 1
    return out, seen_any


def make_room(tag, seed, n, c, box_x, box_y, angle, center, views, size):
    rng = np.random.default_rng(seed)
    center = np.asarray(center, np.float64)
    local = (rng.random((n, 3)) - 0.5) * np.array([box_x, box_y, 2.8])  # about the centre, axis-aligned
    rot_cos, rot_sin = PR.rotation(angle)
    # the raw room is the aligned one turned back: raw = R^T local + centre
    raw = np.stack([local[:, 0] * rot_cos + local[:, 1] * rot_sin, -local[:, 0] * rot_sin + local[:, 1] * rot_cos, local[:, 2]], 1)
    coord = (raw + center).astype(np.float32)
    coord64 = PR.align(coord, angle, center)
    patch = (np.floor((local[:, 0] + box_x / 2) / 1.5).astype(np.int64) * 4 + np.floor((local[:, 1] + box_y / 2) / 1.5).astype(np.int64))
    instance = (patch * 37 + 5).astype(np.int32)          # sparse ids
    semantic = ((patch * 7 + 3) % c).astype(np.int32)
    view_list = make_views(rng, coord64, center, box_x, box_y, views, size)
    quiet = views - 2  # the view that sees points but no weak point
    for _ in range(500):
        found, seen_any = bridges_of(coord64, view_list)
        ids = np.unique(instance)
        inst, sem = instance.copy(), semantic.copy()
        inst[inst == ids[1]] = -1                           # an instance with id -1
        sem[inst == ids[2]] = -1                            # an instance whose ground truth is -1
        unseen, seen = np.nonzero(seen_any == 0)[0], np.nonzero(seen_any == 1)[0]
        inst[unseen[5]] = 2 ** 31 - 2                       # a single point (not seen)
        inst[np.r_[seen[[40, 90]], unseen[10:16]]] = -2 ** 31  # exactly two seen points among eight
        inst[unseen[20:31]] = 70001                         # no view sees it
        weak = PR.weak_mask(inst, seen_any)
        prompts = PR.view_prompts(found[quiet][0], weak, sem)[0]
        if prompts.size == 0:
            break
        xy = found[quiet][0][prompts, :2]
        view_list[quiet]["depth"][xy[:, 1], xy[:, 0]] = int(0.25 * DEPTH_SCALE)  # something stands in front of them
    else:
        raise AssertionError("the quiet view does not settle")
    return dict(tag=tag, seed=seed, n=n, c=c, coord=coord, angle=angle, center=center, instance=inst.reshape(n, 1),
                semantic=sem.reshape(n, 1), views=view_list, size=size, quiet=quiet)


def view_args(case):
    """the `views` argument of pp2s_scene"""
    return [(v["key"], v["k"], v["rt"], v["depth"]) for v in case["views"]]


def masks_for(case, view_key, xy, cls):
    """(P, H, W) bool: a disc around the prompt's own mask element (row y - 1, column x - 1), of a radius drawn from (seed,
    view, x, y, class): neighbouring prompts of different classes overlap, so points collect two classes inside one view."""
    width, height = case["size"]
    rr, cc = np.mgrid[0:height, 0:width]
    out = np.zeros((len(cls), height, width), bool)
    view = int(view_key[4:])
    for p, ((x, y), k) in enumerate(zip(np.asarray(xy).astype(np.int64), np.asarray(cls).astype(np.int64))):
        g = np.random.default_rng([case["seed"], view, int(x), int(y), int(k)])
        radius = g.integers(3, 8)
        out[p] = (rr - (y - 1) % height) ** 2 + (cc - (x - 1) % width) ** 2 <= radius ** 2
    return out


def digest(case):
    h = hashlib.sha256()
    for a in [case["coord"], case["center"], np.int64(case["angle"]), case["instance"], case["semantic"]]:
        h.update(np.ascontiguousarray(a).tobytes())
    for v in case["views"]:
        for a in (v["k"], v["rt"], v["depth"]):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load():
    """{name: array} of tests/golden/pp2s.npz, after checking that the seeded inputs are the ones it was made for"""
    fx = dict(np.load(os.path.join(GOLDEN, "pp2s.npz"), allow_pickle=False))
    for tag in CASES:
        assert str(fx[tag + "_digest"]) == digest(room(tag)), "the seeded inputs of %s are not those of the fixture" % tag
    return fx


def expected(fx, case):
    """the fixture's arrays of a room in the shapes the functions return: bridges [(n, 3) int32] per view (zeros for a view
    without a bridge file), visible, seen_any and weak (n,) uint8, prompts [(idx, xy, cls)] per view, label (n,) int32"""
    tag, n = case["tag"], case["n"]
    bridges, prompts = [], []
    for v in range(len(case["views"])):
        rows = fx["%s_bridge%d" % (tag, v)].astype(np.int64)
        bridge = np.zeros((n, 3), np.int32)
        bridge[rows[:, 0]] = np.concatenate([rows[:, 1:], np.ones((rows.shape[0], 1), np.int64)], 1)
        bridges.append(bridge)
        table = fx["%s_prompts%d" % (tag, v)]
        prompts.append((table[:, 0].astype(np.int64), table[:, 1:3].astype(np.int32), table[:, 3].astype(np.int32)))
    weak = np.zeros(n, np.uint8)
    weak[fx[tag + "_weak"]] = 1
    return dict(aligned=fx[tag + "_aligned"], bridges=bridges, visible=fx[tag + "_visible"].tolist(),
                seen_any=np.unpackbits(fx[tag + "_seen_any"])[:n], weak=weak, prompts=prompts, label=fx[tag + "_label"].astype(np.int32))


def align_bound(case, rows=slice(None)):
    """2 * gamma_3 * sum |a_i| |b_i| per element of the aligned room: the rotation's products (the third is t.z * 1 for z and a
    product with 0 for x and y), gamma_3 = 3u / (1 - 3u), u = 2 ** -53"""
    u = 2.0 ** -53
    rot_cos, rot_sin = PR.rotation(case["angle"])
    t = np.abs((case["coord"].astype(np.float64) - case["center"]).astype(np.float32).astype(np.float64))[rows]
    total = np.stack([t[:, 0] * abs(rot_cos) + t[:, 1] * abs(rot_sin), t[:, 0] * abs(rot_sin) + t[:, 1] * abs(rot_cos), t[:, 2]], 1)
    return 2 * (3 * u / (1 - 3 * u)) * total
