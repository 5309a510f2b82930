"""A vectorised numpy restatement of REAL's epoch-end label refinement, written from the semantics that
include/ptv2_refine_hip.h states (no test in here).  tests/test_refine_host.py pins it to tests/golden/refine.npz, which the
reference's own statements produced; the GPU tests and tools/bench_refine.py use it for shapes the fixture does not hold.
"""
import math

import numpy as np


def confidence(logits, dtype=np.float32):
    """pred (first maximum, -1 for an unseen row), top-two margin of the softmax exp(x - max) / sum computed in `dtype`"""
    logits = np.asarray(logits)
    pred = np.argmax(logits, axis=1).astype(np.int32)
    pred[logits[:, 0] == -100] = -1
    x = logits.astype(dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = np.sort(e / e.sum(axis=1, keepdims=True), axis=1)
    return pred, p[:, -1] - p[:, -2]


def grid_cells(lo_x, hi_x, lo_y, hi_y, grid=0.5):
    lx, ly = np.float32(hi_x) - np.float32(lo_x), np.float32(hi_y) - np.float32(lo_y)
    return max(int(math.ceil(lx) // grid), 0), max(int(math.ceil(np.floor_divide(ly, np.float32(grid)))), 0)


def cells_of(x, lo, cells, grid):
    """cell of every x, -1 for none: bound(i) = float32(lo) + float32(i * grid), both ends strict"""
    bound = np.float32(lo) + (np.arange(cells + 1, dtype=np.float64) * grid).astype(np.float32)
    j = np.searchsorted(bound, x, side="left")  # bound[j - 1] < x <= bound[j]
    ok = (j >= 1) & (j <= cells)
    ok &= x < bound[np.minimum(j, cells)]
    return np.where(ok, j - 1, -1)


def prompts(coord, pred, conf, label, present, grid=0.5, threshold=0.9, groups=False):
    """(prompt_idx, prompt_cls) in (x cell, y cell, class) order; groups=True also returns {(ix, iy, class): candidate rows}"""
    coord = np.asarray(coord, np.float32)
    n, c = coord.shape[0], len(present)
    label = np.asarray(label).reshape(-1)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    if n == 0:
        return empty + ({},) if groups else empty
    lo, hi = coord.min(axis=0), coord.max(axis=0)
    nx, ny = grid_cells(lo[0], hi[0], lo[1], hi[1], grid)
    if nx == 0 or ny == 0:
        return empty + ({},) if groups else empty
    ix, iy = cells_of(coord[:, 0], lo[0], nx, grid), cells_of(coord[:, 1], lo[1], ny, grid)
    k = pred.astype(np.int64)
    cand = (ix >= 0) & (iy >= 0) & (k >= 0) & (conf > np.float32(threshold)) & (label != k)
    cand &= np.asarray(present, bool)[np.clip(k, 0, c - 1)]
    rows = np.nonzero(cand)[0]
    key = (ix[rows] * ny + iy[rows]) * c + k[rows]
    order = np.lexsort((rows, -conf[rows].astype(np.float64), key))  # by key, then conf descending, then index ascending
    rows, key = rows[order], key[order]
    first = np.ones(rows.size, bool)
    first[1:] = key[1:] != key[:-1]
    out = rows[first].astype(np.int32), (key[first] % c).astype(np.int32)
    if not groups:
        return out
    starts = np.nonzero(first)[0].tolist() + [rows.size]
    return out + ({int(key[a]): rows[a:b] for a, b in zip(starts[:-1], starts[1:])},)


def inside_points(bridge, masks):
    """rows (V,) of the visible points and inside (P, V): which of them each mask holds (mask[u - 1][v - 1], [0][0] cleared)"""
    bridge = np.asarray(bridge).astype(np.int64)
    height, width = masks.shape[1:]
    rows = np.nonzero(bridge[:, 2] == 1)[0]
    u, v = bridge[rows, 0], bridge[rows, 1]
    if ((u < 0) | (u > height) | (v < 0) | (v > width)).any():
        raise IndexError("a visible point's pixel lies outside the image")
    r, q = np.where(u == 0, height - 1, u - 1), np.where(v == 0, width - 1, v - 1)
    return rows, (np.asarray(masks)[:, r, q] != 0) & ((r != 0) | (q != 0))[None, :]


def vote_view(vote, bridge, pred, conf, prompt_idx, prompt_cls, masks_for, threshold=0.9):
    """adds one view's votes into vote (n, c); returns the number of prompts the view saw (masks_for is called when > 0)"""
    bridge = np.asarray(bridge)
    seen = np.nonzero(bridge[prompt_idx, 2] == 1)[0]
    if seen.size == 0:
        return 0
    cls = prompt_cls[seen]
    masks = np.asarray(masks_for(bridge[prompt_idx[seen], :2].astype(np.float32), cls))
    rows, inside = inside_points(bridge, masks)
    c = vote.shape[1]
    hot = conf[rows] > np.float32(threshold)
    for p in range(seen.size):
        hist = np.bincount(pred[rows][inside[p] & hot], minlength=c)
        if hist.sum() > 0 and int(np.argmax(hist)) == int(cls[p]):
            vote[rows[inside[p]], cls[p]] += 1
    return int(seen.size)


def update(vote, pred, label):
    """(new label, number of labels changed)"""
    label = np.array(label).reshape(-1)
    result = np.argmax(vote, axis=1)
    valid = (vote.sum(axis=1) != 0) & (result == pred) & (pred != -1)
    count = int((label[valid] != result[valid]).sum())
    label[valid] = result[valid]
    return label, count


def refine_scene(logits, coord, label, present, views, masks_for, grid=0.5, threshold=0.9):
    """dict(pred, conf, prompt_idx, prompt_cls, vote, label, updated, touched, seen); views: (bridge, key) pairs;
    masks_for(key, pixel_uv, prompt_cls)"""
    pred, conf = confidence(logits)
    label = np.asarray(label).reshape(-1)
    prompt_idx, prompt_cls = prompts(coord, pred, conf, label, present, grid, threshold)
    vote = np.zeros((pred.shape[0], len(present)), np.int32)
    seen = [vote_view(vote, bridge, pred, conf, prompt_idx, prompt_cls, lambda uv, k, _key=key: masks_for(_key, uv, k), threshold)
            for bridge, key in views]
    touched = any(s > 0 for s in seen)
    new_label, updated = update(vote, pred, label) if touched else (label.copy(), 0)
    return dict(pred=pred, conf=conf, prompt_idx=prompt_idx, prompt_cls=prompt_cls, vote=vote, label=new_label, updated=updated,
                touched=touched, seen=np.asarray(seen))
