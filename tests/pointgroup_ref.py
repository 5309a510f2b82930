"""numpy restatement of PointGroup's clustering stage, written from the semantics (include/ptv2_pg_hip.h):
a brute-force ball query with the cap, the directed breadth-first search, proposals and scores in float64, both offset losses
and their gradient in float64.  The yardstick of tests/test_pointgroup_host.py and tests/test_gpu_pointgroup*.py, and what the
`pointgroup_ops` stub of tests/golden/make_golden_pointgroup.py calls."""
import collections

import numpy as np

BALL_CAP = 1000


def pair_d2(coords, lo, hi):
    """(hi - lo, hi - lo) float64 squared distances of the fp32 coordinates of one segment"""
    seg = np.asarray(coords[lo:hi], np.float32).astype(np.float64)
    d = seg[:, None, :] - seg[None, :, :]
    return (d * d).sum(-1)


def ball_query(coords, batch_offsets, radius, cap=BALL_CAP):
    """(lists, idx, start_len, capped): lists[p] the ascending indices k of p's segment with d2(p, k) < radius^2 (strict, p
    included), the first `cap`; idx their concatenation in point order, start_len (n, 2) with start the exclusive prefix sum of
    len; capped: some point had more than `cap`"""
    n = coords.shape[0]
    lists, capped = [None] * n, False
    r2 = float(np.float32(radius)) ** 2
    for s in range(len(batch_offsets) - 1):
        lo, hi = int(batch_offsets[s]), int(batch_offsets[s + 1])
        if hi <= lo:
            continue
        near = pair_d2(coords, lo, hi) < r2
        for p in range(lo, hi):
            hits = np.nonzero(near[p - lo])[0] + lo
            capped = capped or hits.shape[0] > cap
            lists[p] = hits[:cap].astype(np.int32)
    lens = np.array([v.shape[0] for v in lists], np.int32).reshape(-1)
    start = (np.cumsum(lens) - lens).astype(np.int32)
    idx = np.concatenate(lists).astype(np.int32) if n else np.zeros(0, np.int32)
    return lists, idx, np.stack([start, lens], 1).astype(np.int32).reshape(-1, 2), capped


def margin(coords, batch_offsets, radius):
    """the smallest |d2 - r^2| / r^2 over the pairs of a segment"""
    r2, best = float(radius) ** 2, np.inf
    for s in range(len(batch_offsets) - 1):
        lo, hi = int(batch_offsets[s]), int(batch_offsets[s + 1])
        if hi > lo:
            best = min(best, float(np.abs(pair_d2(coords, lo, hi) - r2).min()) / r2)
    return best


def bfs_cluster(label, idx, start_len, threshold):
    """(cluster_idxs (sum, 2), cluster_offsets (nCluster + 1)) int32: seeds in ascending index; a queue; the entries of the
    current point's list in list order; an entry joins when it carries the current point's label and no search has visited
    it; sets of at least `threshold` points are kept, their members in the order they were found"""
    n = start_len.shape[0]
    visited = np.zeros(n, bool)
    rows, offsets = [], [0]
    for seed in range(n):
        if visited[seed]:
            continue
        visited[seed] = True
        found, todo = [seed], collections.deque([seed])
        while todo:
            cur = todo.popleft()
            start, length = int(start_len[cur, 0]), int(start_len[cur, 1])
            for k in idx[start:start + length]:
                if not visited[k] and label[k] == label[cur]:
                    visited[k] = True
                    found.append(int(k))
                    todo.append(int(k))
        if len(found) >= threshold:
            rows += [(len(offsets) - 1, k) for k in found]
            offsets.append(offsets[-1] + len(found))
    return np.array(rows, np.int32).reshape(-1, 2), np.array(offsets, np.int32)


def point_cluster(rows, n):
    out = np.full(n, -1, np.int32)
    out[rows[:, 1]] = rows[:, 0]
    return out


def softmax64(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def proposals(rows, offsets, segment_pred, prob, propose_points, n):
    """(scores float64 (P), masks int32 (P, n), classes int64 (P), members (P)) of the clusters with more than propose_points
    members, in cluster order: the class of a cluster's first point, the mean of prob[:, class] over its members"""
    scores, masks, classes, members = [], [], [], []
    for c in range(len(offsets) - 1):
        pts = rows[offsets[c]:offsets[c + 1], 1]
        if pts.shape[0] <= propose_points:
            continue
        cls = int(segment_pred[pts[0]])
        mask = np.zeros(n, np.int32)
        mask[pts] = 1
        scores.append(float(np.asarray(prob, np.float64)[pts, cls].mean()))
        masks.append(mask)
        classes.append(cls)
        members.append(pts.shape[0])
    return (np.array(scores, np.float64), np.array(masks, np.int32).reshape(-1, n), np.array(classes, np.int64),
            np.array(members, np.int64))


def propose(coord, offset, bias_pred, logit_pred, ignore, thresh, min_points, propose_points, voxel_size):
    """the evaluation branch of the model in float64 from fp32 inputs: (scores, masks, classes, members, margin); margin is the
    ball query's over the shifted points that are clustered (inf when none is)"""
    n = coord.shape[0]
    prob = softmax64(logit_pred)
    segment_pred = prob.argmax(1)
    center = ((coord.astype(np.float32) + bias_pred.astype(np.float32)) / np.float32(voxel_size)).astype(np.float32)
    keep = np.nonzero(~np.isin(segment_pred, list(ignore)))[0]
    if keep.shape[0] == 0:
        return np.zeros(0), np.zeros((0, n), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.inf
    batch = np.searchsorted(np.asarray(offset), keep, side="right")
    offset_ = np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=len(offset)))]).astype(np.int32)
    _, idx, start_len, _ = ball_query(center[keep], offset_, thresh)
    rows, offsets = bfs_cluster(segment_pred[keep], idx, start_len, min_points)
    rows = rows.copy()
    rows[:, 1] = keep[rows[:, 1]]
    return proposals(rows, offsets, segment_pred, prob, propose_points, n) + (margin(center[keep], offset_, thresh),)


def bias_loss(bias_pred, coord, instance_center, instance, ignore, g_l1=1.0, g_cos=1.0):
    """(bias_l1_loss, bias_cosine_loss, d bias_pred) in float64.  The gradient follows torch's autograd of the reference's
    statements: sign(0) = 0 in the L1 term; the gradient of the norm at the zero vector is 0, so a zero row gets
    g * gt_norm / 1e-8 from the quotient alone; ignored rows get 0."""
    p = np.asarray(bias_pred, np.float64)
    gt = np.asarray(instance_center, np.float64) - np.asarray(coord, np.float64)
    mask = (np.asarray(instance) != ignore).astype(np.float64)
    denom = mask.sum() + 1e-8
    l1 = (np.abs(p - gt).sum(1) * mask).sum() / denom
    norm_p = np.sqrt((p * p).sum(1, keepdims=True))
    norm_g = np.sqrt((gt * gt).sum(1, keepdims=True))
    pn, gn = p / (norm_p + 1e-8), gt / (norm_g + 1e-8)
    cos = (-(pn * gn).sum(1) * mask).sum() / denom
    a = norm_p + 1e-8
    dot = (p * gn).sum(1, keepdims=True)
    unit = np.divide(p, norm_p, out=np.zeros_like(p), where=norm_p > 0)
    d_cos = -(gn / a - dot * unit / (a * a))
    grad = (g_l1 * np.sign(p - gt) + g_cos * d_cos) * mask[:, None] / denom
    return l1, cos, grad
