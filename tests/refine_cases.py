"""Seeded synthetic rooms, bridges and masks shared by tests/golden/make_golden_refine.py, tests/test_refine_host.py,
tests/test_gpu_refine.py and tools/bench_refine.py (no test in here).  Everything is built on the CPU with numpy from a seed;
the fixture (tests/golden/refine.npz) stores the reference's OUTPUTS for these inputs and a digest of the inputs, which
`load()` compares, so that a numpy whose generators drew other numbers fails loudly instead of comparing against the wrong room.

A room: points uniform in a box, a "true" class per 1.5 m patch of the floor plan, logits that are multiples of 1/4 (no
softmax saturates: |x| <= 12), a block of unseen rows (-100), a block of rows duplicated bit for bit next to their originals
(exact ties inside a cell), pseudo-labels that disagree with the prediction on about a third of the points.  A view maps a
window of the floor plan linearly onto the pixels, so that a disc of pixels is a patch of neighbouring points.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID, THRESHOLD = 0.5, 0.9

#        tag: (seed, points, classes, box x, box y, absent classes, views, height, width)
CASES = {"c13": (11, 4000, 13, 6.3, 4.6, (5,), 4, 48, 64),
         "c20": (23, 3000, 20, 4.2, 5.4, (0, 17), 3, 40, 56)}


def room(tag):
    return make_room(tag, *CASES[tag])


def blocks(n):
    """(unseen rows, the duplicated block, its copy at higher indices, its copy at lower indices)"""
    src = np.arange(n // 4, n // 4 + max(n // 100, min(4, n // 8)))
    return np.arange(int(0.075 * n), int(0.085 * n)), src, src + (3 * n) // 8, src - n // 8


def make_room(tag, seed, n, c, box_x, box_y, absent=(), views=2, height=12, width=16, flat=(2.0, 4.5, 7.0, 9.5, 12.0), settled=True):
    rng = np.random.default_rng(seed)
    coord = (rng.random((n, 3)) * np.array([box_x, box_y, 3.0])).astype(np.float32)
    coord[:, 0] += np.float32(1.0)
    patch = (np.floor((coord[:, 0] - 1.0) / 1.5).astype(np.int64) * 5 + np.floor(coord[:, 1] / 1.5).astype(np.int64))
    allowed = np.array([k for k in range(c) if k not in absent])
    true = allowed[(patch * 7 + 3) % allowed.size]
    pred_cls = np.where(rng.random(n) < 0.12, rng.integers(0, c, n), true)  # some rows predict another class (absent ones too)
    logits = rng.integers(-8, 9, (n, c)).astype(np.float32) / 4
    lead = rng.choice(np.array(flat, np.float32), n)
    logits[np.arange(n), pred_cls] = lead
    unseen, src, higher, lower = blocks(n)
    logits[unseen] = -100.0
    # the duplicated block: the sharpest row a scene holds, twice in one spot (the copy at the HIGHER index, and once more at
    # a LOWER index than its original), so that a (cell, class) group is led by an exact tie
    for dst in (higher, lower):
        logits[src] = -2.0
        logits[src, true[src]] = 12.0
        logits[dst] = logits[src]
        coord[dst] = coord[src] + np.float32(0.001)
    label = np.where(rng.random(n) < 0.35, rng.integers(0, c, n), true).astype(np.int64)
    dup = np.concatenate([src, higher, lower])
    label[dup] = (true[np.concatenate([src, src, src])] + 1) % c  # all three disagree with the prediction: candidates
    present = np.zeros(c, np.uint8)
    present[allowed] = 1
    if settled:  # (a timing run does not compare choices)
        settle(coord, logits, label, present)
    from tests import refine_ref as RR

    pred, conf = RR.confidence(logits)
    prompt_rows = RR.prompts(coord, pred, conf, label, present, GRID, THRESHOLD)[0]
    bridges = []
    for v in range(views):
        x0, y0 = 1.0 + 0.13 * box_x * v, 0.09 * box_y * v
        span_x, span_y = 0.57 * box_x, 0.67 * box_y
        u = np.floor((coord[:, 0] - x0) / span_x * height).astype(np.int64) + 1
        w = np.floor((coord[:, 1] - y0) / span_y * width).astype(np.int64) + 1
        seen = (u >= 1) & (u <= height) & (w >= 1) & (w <= width) & (rng.random(n) < 0.8)
        if v == views - 1:
            seen[prompt_rows] = False  # the last view sees points, but none that is a prompt
        wrap = seen & (rng.random(n) < 0.03)
        u[wrap] = 0  # numpy's index -1: the last row
        wrap = seen & (rng.random(n) < 0.03)
        w[wrap] = 0
        u[~seen], w[~seen] = 10 ** 6, -7  # never read: the point is not visible
        bridges.append(np.stack([u, w, seen.astype(np.int64)], 1))
    return dict(tag=tag, n=n, c=c, coord=coord, logits=logits, label=label.reshape(n, 1), present=present,
                classes=np.nonzero(present)[0], bridges=bridges, height=height, width=width, seed=seed)


def rivals(coord, logits, label, present):
    """rows that make the reference's choice depend on rounding: a confidence within 1e-4 of the threshold, or in a (cell,
    class) group the first row that is not a bit-for-bit copy of the winner, when its float64 confidence is not more than
    2e-5 below the winner's (the fixture's condition asks for 1e-5)"""
    from tests import refine_ref as RR

    pred, conf = RR.confidence(logits)
    conf64 = RR.confidence(logits, np.float64)[1]
    out = np.nonzero((np.abs(conf64 - THRESHOLD) <= 2e-4) | (np.abs(conf - np.float32(THRESHOLD)) <= 2e-4))[0].tolist()
    groups = RR.prompts(coord, pred, conf, label, present, GRID, THRESHOLD, groups=True)[2]
    for rows in groups.values():
        other = [r for r in rows[1:] if not np.array_equal(logits[r], logits[rows[0]])]
        if other and conf64[rows[0]] - conf64[other[0]] <= 2e-5:
            out.append(other[0])
    return np.asarray(out, np.int64), pred


def settle(coord, logits, label, present):
    """flattens the leading logit of every rival row (it stops being a candidate) until none is left"""
    for _ in range(100):
        rows, pred = rivals(coord, logits, label, present)
        if rows.size == 0:
            return
        logits[rows, pred[rows]] = 2.0
    raise AssertionError("the room does not settle")


def masks_for(case, view, pixel_uv, prompt_cls):
    """(P, H, W) bool: a disc around the prompt's own mask element (row u - 1, column v - 1, wrapped as numpy does), of a
    radius drawn from (seed, view, u, v, class); every third mask also holds the element [0, 0] and the last row."""
    height, width = case["height"], case["width"]
    rr, cc = np.mgrid[0:height, 0:width]
    out = np.zeros((len(prompt_cls), height, width), bool)
    for p, ((u, v), k) in enumerate(zip(np.asarray(pixel_uv).astype(np.int64), np.asarray(prompt_cls).astype(np.int64))):
        g = np.random.default_rng([case["seed"], view, int(u), int(v), int(k)])
        r0, c0 = (u - 1) % height, (v - 1) % width
        radius = g.integers(3, 10)
        out[p] = (rr - r0) ** 2 + (cc - c0) ** 2 <= radius ** 2
        if g.integers(0, 3) == 0:
            out[p, 0, 0] = True
            out[p, height - 1, :] = True
    return out


def digest(case):
    h = hashlib.sha256()
    for a in [case["coord"], case["logits"], case["label"], case["present"]] + case["bridges"]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load():
    """{name: array} of tests/golden/refine.npz, after checking that the seeded inputs are the ones it was made for"""
    fx = dict(np.load(os.path.join(GOLDEN, "refine.npz"), allow_pickle=False))
    for tag in CASES:
        assert str(fx[tag + "_digest"]) == digest(room(tag)), "the seeded inputs of %s are not those of the fixture" % tag
    return fx
