"""tests/msc_ref.py -- Masked Scene Contrast (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py) restated
in numpy: the patch ids and cross masks (:94-141), the pair matching after the kNN (:154-172) and the losses (:179-193, :281-305)
in float64.  Offsets are the reference's ascending scene ends.  No torch, no GPU: the reference the GPU tests and
tests/golden/make_golden_msc.py compare against.
"""
import numpy as np


def offset2batch(offset, n):
    return np.searchsorted(np.asarray(offset, np.int64), np.arange(n), side="right")


# ------------------------------------------------------------------------------------------------------- cross masks ----
def cells(origin, grid):
    """floor(origin / grid) in fp32, IEEE division (:94-95)"""
    return np.floor(np.asarray(origin, np.float32) / np.float32(grid))


def voxel_grid_ids(cell, batch):
    """oracle/ptv2_ref.py::voxel_grid(pos=cell, size=1, batch, start=0): id = sum_d trunc(p_d) prod_{e<d} (trunc(max_e) + 1)
    over p = (cell, batch), int64.  Cells are not shifted: a negative cell can share its id with another one."""
    p = np.concatenate([cell.astype(np.float32), batch.reshape(-1, 1).astype(np.float32)], 1)
    num = np.trunc(p.max(0)).astype(np.int64) + 1
    stride = np.concatenate([[1], np.cumprod(num)])[:4]
    return (np.trunc(p).astype(np.int64) * stride[None, :]).sum(1)


def patch_ids(origin1, offset1, origin2, offset2, grid):
    """(n1 + n2) int64: view 1, then view 2, the maxima over both"""
    cell = np.concatenate([cells(origin1, grid), cells(origin2, grid)])
    batch = np.concatenate([offset2batch(offset1, len(origin1)), offset2batch(offset2, len(origin2))])
    return voxel_grid_ids(cell, batch)


def alias_free_ids(origin1, offset1, origin2, offset2, grid):
    """one id per distinct (cell, scene): what a partition without the aliasing would be"""
    cell = np.concatenate([cells(origin1, grid), cells(origin2, grid)])
    batch = np.concatenate([offset2batch(offset1, len(origin1)), offset2batch(offset2, len(origin2))])
    rows = np.concatenate([cell.astype(np.int64), batch.reshape(-1, 1)], 1)
    return np.unique(rows, axis=0, return_inverse=True)[1].reshape(-1)


def masks_of_ids(ids, n1, mask_rate, perm):
    unique, cluster = np.unique(ids, return_inverse=True)
    patch_num = len(unique)
    m = int(patch_num * mask_rate)
    tag = np.zeros(patch_num, np.int32)
    perm = np.asarray(perm, np.int64)
    tag[perm[0:m]] = 1
    tag[perm[m:2 * m]] = 2
    point = tag[cluster.reshape(-1)]
    return point[:n1] == 1, point[n1:] == 2


def cross_masks(origin1, offset1, origin2, offset2, grid, mask_rate, perm):
    """(mask1 (n1), mask2 (n2)) bool; perm: a permutation of the patches, which are numbered by ascending id"""
    assert mask_rate <= 0.5
    return masks_of_ids(patch_ids(origin1, offset1, origin2, offset2, grid), len(origin1), mask_rate, perm)


def patch_count(origin1, offset1, origin2, offset2, grid):
    return len(np.unique(patch_ids(origin1, offset1, origin2, offset2, grid)))


# ---------------------------------------------------------------------------------------------------------- matching ----
def knn_bruteforce(k, xyz, offset, new_xyz, new_offset):
    """(idx (m, k) int32, dist2 (m, k) fp32) of the k nearest points of xyz in the same scene; -1 / 1e10 where a scene has fewer.
    Squared distances as the kernels round them: fma(dz, dz, fma(dx, dx, dy * dy)) in fp32 (the float64 sums below round once
    more only when a sum needs over 53 bits).  Equal distances: ascending index."""
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    m = len(new_xyz)
    idx = np.full((m, k), -1, np.int32)
    dist2 = np.full((m, k), 1e10, np.float32)
    scene = offset2batch(new_offset, m)
    starts = np.concatenate([[0], np.asarray(offset, np.int64)])
    for i in range(m):
        lo, hi = starts[scene[i]], starts[scene[i] + 1]
        d = new_xyz[i][None, :] - xyz[lo:hi]  # fp32
        yy = (d[:, 1] * d[:, 1]).astype(np.float32)
        inner = (d[:, 0].astype(np.float64) * d[:, 0].astype(np.float64) + yy.astype(np.float64)).astype(np.float32)
        d2 = (d[:, 2].astype(np.float64) * d[:, 2].astype(np.float64) + inner.astype(np.float64)).astype(np.float32)
        order = np.argsort(d2, kind="stable")[:k]
        idx[i, :len(order)] = order + lo
        dist2[i, :len(order)] = d2[order]
    return idx, dist2


def match(idx, dist2, max_radius, row_draws):
    """(P, 2) int64 in ascending view-1 row order: per row with a hit (idx >= 0 and sqrt(dist2) < max_radius in fp32, strict) the
    hit of rank count - 1 - row_draws[row] % count in column order (:154-169 when the draw of that row is row_draws[row])"""
    hit = (np.asarray(idx) >= 0) & (np.sqrt(np.asarray(dist2, np.float32)) < np.float32(max_radius))
    out = []
    for i in range(len(idx)):
        cols = np.nonzero(hit[i])[0]
        if len(cols):
            out.append((i, int(idx[i, cols[len(cols) - 1 - int(row_draws[i]) % len(cols)]])))
    return np.asarray(out, np.int64).reshape(-1, 2)


def hit_counts(idx, dist2, max_radius):
    return ((np.asarray(idx) >= 0) & (np.sqrt(np.asarray(dist2, np.float32)) < np.float32(max_radius))).sum(1)


def cut_pairs(pairs, max_pair, perm):
    """:170-171"""
    if len(pairs) > max_pair:
        return pairs[np.asarray(perm, np.int64)[:max_pair]]
    return pairs


def spread_draws(idx, dist2, max_radius, matched_draws):
    """the reference draws one value per matched row: spread those onto all rows (0 elsewhere)"""
    rows = np.nonzero(hit_counts(idx, dist2, max_radius) > 0)[0]
    assert len(rows) == len(matched_draws)
    out = np.zeros(len(idx), np.int64)
    out[rows] = np.asarray(matched_draws, np.int64)
    return out


# ------------------------------------------------------------------------------------------------------------ losses ----
def info_nce(f1, f2, pairs, t, g=1.0):
    """float64: dict(loss, pos_sim, neg_sim, df1, df2, df1_pos, df2_pos), the gradients those of g * loss; df*_pos those of its
    positive term alone, g * mean_i(-a_i.b_i / t): the loss is that term plus the mean log-sum-exp, and the two cancel
    (exactly at M = 1), so an error is measured against the larger of the result and this term"""
    f1, f2, pairs = np.asarray(f1, np.float64), np.asarray(f2, np.float64), np.asarray(pairs, np.int64)
    m = len(pairs)
    x, y = f1[pairs[:, 0]], f2[pairs[:, 1]]
    nx, ny = np.sqrt((x * x).sum(1, keepdims=True)), np.sqrt((y * y).sum(1, keepdims=True))
    a, b = x / (nx + 1e-7), y / (ny + 1e-7)
    sim = a @ b.T
    pos_sim = np.diagonal(sim).mean()
    neg_sim = sim.mean(-1).mean() - pos_sim / m
    s = sim / t
    mx = s.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(s - mx).sum(1))
    loss = (lse - np.diagonal(s)).mean()
    p = np.exp(s - lse[:, None])
    d = (p - np.eye(m)) * (g / (m * t))
    da, db = d @ b, d.T @ a

    def through_norm(dn, unit, norm):
        with np.errstate(divide="ignore", invalid="ignore"):
            second = np.where(norm > 0, unit * (dn * unit).sum(1, keepdims=True) / norm, 0.0)
        return dn / (norm + 1e-7) - second

    df1, df2, df1_pos, df2_pos = np.zeros_like(f1), np.zeros_like(f2), np.zeros_like(f1), np.zeros_like(f2)
    np.add.at(df1, pairs[:, 0], through_norm(da, a, nx))
    np.add.at(df2, pairs[:, 1], through_norm(db, b, ny))
    np.add.at(df1_pos, pairs[:, 0], through_norm(-b * (g / (m * t)), a, nx))
    np.add.at(df2_pos, pairs[:, 1], through_norm(-a * (g / (m * t)), b, ny))
    return dict(loss=loss, pos_sim=pos_sim, neg_sim=neg_sim, df1=df1, df2=df2, df1_pos=df1_pos, df2_pos=df2_pos)


def color_loss(pred1, color1, pred2, color2):
    """:281-284 over the masked rows"""
    pred1, color1, pred2, color2 = (np.asarray(v, np.float64) for v in (pred1, color1, pred2, color2))
    return (((pred1 - color1) ** 2).sum() + ((pred2 - color2) ** 2).sum()) / (len(pred1) + len(pred2))


def normal_loss(pred1, normal1, pred2, normal2):
    """:296-305 over the masked rows (the reference's sign: a plain sum of dot products)"""
    pred1, normal1, pred2, normal2 = (np.asarray(v, np.float64) for v in (pred1, normal1, pred2, normal2))
    pred1 = pred1 / (np.sqrt((pred1 * pred1).sum(1, keepdims=True)) + 1e-10)
    pred2 = pred2 / (np.sqrt((pred2 * pred2).sum(1, keepdims=True)) + 1e-10)
    return ((pred1 * normal1).sum() + (pred2 * normal2).sum()) / (len(pred1) + len(pred2))
