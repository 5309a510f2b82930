"""Masked Scene Contrast's operators on ao_amd/csrc/msc.hip (C ABI include/ptv2_msc_hip.h) and, for
MSC-v1m2 (CSC), on ao_amd/csrc/msc_csc.hip (include/ptv2_csc_hip.h; section 16): `csc_nce`, the partitioned InfoNCE loss.

`info_nce`, `match_pairs` and `cross_masks` are what ao_amd/msc/model.py calls: the contrastive loss over matched pairs without
the (M, M) similarity matrix, the choice of one matched view-2 point per view-1 point after the kNN, and the two cross masks
from the patch ids of the union of both views.  Offsets are the reference's: the ascending scene ends, shape (b).

AO_AMD_MSC=torch (read on every call) is the A/B path: the reference's eager statements on the device, the materialised `sim`
included.  It takes the same draws and returns the same values.
"""
import ctypes
import os

import torch

from .. import _abi, _lib
from ..pointops.query import knn_query_dist2

MAX_PAIRS = _abi.msc_consts["MSC_MAX_PAIRS"]
MAX_CHANNELS = _abi.msc_consts["MSC_MAX_CHANNELS"]
MAX_K = _abi.msc_consts["MSC_MAX_K"]
CSC_MAX_PAIRS = _abi.csc_consts["CSC_MAX_PAIRS"]
CSC_MAX_CHANNELS = _abi.csc_consts["CSC_MAX_CHANNELS"]
CSC_MAX_SCENES = _abi.csc_consts["CSC_MAX_SCENES"]
CSC_CLASSES = _abi.csc_consts["CSC_CLASSES"]
CSC_MAX_INV_T = _abi.csc_consts["CSC_MAX_INV_T"]


def use_hip():
    return os.environ.get("AO_AMD_MSC", "hip") != "torch"


# ---------------------------------------------------------------------------------------------------------- InfoNCE ----
def info_nce_torch(view1_feat, view2_feat, match_index, nce_t):
    """masked_scene_contrast_v1m1_base.py:179-193, statement for statement"""
    view1_feat = view1_feat[match_index[:, 0]]
    view2_feat = view2_feat[match_index[:, 1]]
    view1_feat = view1_feat / (torch.norm(view1_feat, p=2, dim=1, keepdim=True) + 1e-7)
    view2_feat = view2_feat / (torch.norm(view2_feat, p=2, dim=1, keepdim=True) + 1e-7)
    sim = torch.mm(view1_feat, view2_feat.transpose(1, 0))
    with torch.no_grad():
        pos_sim = torch.diagonal(sim).mean()
        neg_sim = sim.mean(dim=-1).mean() - pos_sim / match_index.shape[0]
    labels = torch.arange(sim.shape[0], device=view1_feat.device).long()
    loss = torch.nn.functional.cross_entropy(torch.div(sim, nce_t), labels, reduction="mean")
    return loss, pos_sim, neg_sim


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, view1_feat, view2_feat, pairs, nce_t):
        f1, f2 = view1_feat.contiguous(), view2_feat.contiguous()
        (n1, c), n2, m, dev = f1.shape, f2.shape[0], pairs.shape[0], f1.device
        L = _lib.lib()
        a = torch.empty((m, c), dtype=torch.float32, device=dev)
        b = torch.empty((m, c), dtype=torch.float32, device=dev)
        norms = torch.empty((2, m), dtype=torch.float32, device=dev)
        lse = torch.empty(m, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _lib.workspace(L.ptv2_msc_nce_workspace_bytes(m, c), dev)
        rc = L.msc_nce_fwd_hip_launcher(n1, n2, m, c, f1.data_ptr(), f2.data_ptr(), pairs.data_ptr(), nce_t, a.data_ptr(),
                                        b.data_ptr(), norms.data_ptr(), lse.data_ptr(), out.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "msc_nce_fwd_hip_launcher")  # (no read-back: a pair outside its operand turns the three outputs NaN)
        ctx.save_for_backward(pairs, a, b, norms, lse)
        ctx.sizes = (n1, n2, nce_t)
        loss, pos_sim, neg_sim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(pos_sim, neg_sim)
        return loss, pos_sim, neg_sim

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, g_pos, g_neg):
        pairs, a, b, norms, lse = ctx.saved_tensors
        n1, n2, nce_t = ctx.sizes
        (m, c), dev = a.shape, a.device
        L = _lib.lib()
        # the order in which the rows of one index are summed: a stable sort of either column
        order = torch.stack([torch.sort(pairs[:, 0], stable=True)[1], torch.sort(pairs[:, 1], stable=True)[1]]).int().contiguous()
        g = g_loss.float().reshape(1).contiguous()
        df1 = torch.empty((n1, c), dtype=torch.float32, device=dev)
        df2 = torch.empty((n2, c), dtype=torch.float32, device=dev)
        ws = _lib.workspace(L.ptv2_msc_nce_workspace_bytes(m, c), dev)
        rc = L.msc_nce_bwd_hip_launcher(n1, n2, m, c, pairs.data_ptr(), order.data_ptr(), nce_t, a.data_ptr(), b.data_ptr(),
                                        norms.data_ptr(), lse.data_ptr(), g.data_ptr(), df1.data_ptr(), df2.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "msc_nce_bwd_hip_launcher")
        return df1, df2, None, None


def info_nce(view1_feat, view2_feat, match_index, nce_t):
    """(loss, pos_sim, neg_sim) of view1_feat (n1, C), view2_feat (n2, C) and match_index (M, 2), in fp32 (under autocast too):
    with a_i, b_i the rows the pairs name, each divided by its norm + 1e-7, loss = mean_i(logsumexp_j(a_i.b_j / t) - a_i.b_i / t),
    pos_sim = mean_i a_i.b_i, neg_sim = mean_ij a_i.b_j - pos_sim / M.  Only the loss carries a gradient.  1 <= M <= MAX_PAIRS
    and C a multiple of 4 up to MAX_CHANNELS run on the tiled kernels, which never hold an (M, M) array; any other size takes
    the eager statements.  M = 0 raises (the reference returns NaN).  A pair that names a row outside its operand makes the
    three outputs NaN on the kernels (nothing is read back to raise on) and contributes no gradient."""
    _lib.require_cuda(view1_feat, view2_feat, match_index)
    if view1_feat.dim() != 2 or view2_feat.dim() != 2 or view1_feat.shape[1] != view2_feat.shape[1] or match_index.dim() != 2 \
            or match_index.shape[1] != 2 or match_index.is_floating_point():
        raise ValueError("ao_amd msc: info_nce takes (n1, C), (n2, C) and integer (M, 2); got %s %s %s %s" % (
            tuple(view1_feat.shape), tuple(view2_feat.shape), tuple(match_index.shape), match_index.dtype))
    m, c = match_index.shape[0], view1_feat.shape[1]
    if m == 0:
        raise ValueError("ao_amd msc: info_nce of no pair (the loss is a mean over the pairs)")
    if not float(nce_t) > 0:
        raise ValueError("ao_amd msc: nce_t %r (> 0)" % (nce_t,))
    pairs = match_index.long().contiguous()
    fits = m <= MAX_PAIRS and 4 <= c <= MAX_CHANNELS and c % 4 == 0 and view1_feat.shape[0] > 0 and view2_feat.shape[0] > 0
    if not use_hip() or not fits:
        with torch.autocast("cuda", enabled=False):
            return info_nce_torch(view1_feat.float(), view2_feat.float(), pairs, float(nce_t))
    return _InfoNCE.apply(view1_feat, view2_feat, pairs, float(nce_t))


# ------------------------------------------------------------------------------------------- partitioned InfoNCE (CSC) ----
def _offset2batch(offset, n):
    return torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)


def compute_partitions_torch(coord1, coord2, r1, r2):
    """masked_scene_contrast_v1m2_csc.py:182-200, statement for statement"""
    partition_matrix = torch.zeros((coord1.shape[0], coord2.shape[0]), device=coord1.device)
    partition_matrix = partition_matrix - 1e7

    rel_trans = coord1.unsqueeze(0) - coord2.unsqueeze(1)
    mask_up = rel_trans[:, :, 2] > 0.0
    mask_down = rel_trans[:, :, 2] < 0.0

    distance_matrix = torch.sqrt(torch.sum(rel_trans.pow(2), 2).add(1e-7))

    mask = (distance_matrix[:, :] > r1) & (distance_matrix[:, :] <= r2)
    partition_matrix[mask & mask_up] = 0
    partition_matrix[mask & mask_down] = 1

    mask = distance_matrix[:, :] > r2
    partition_matrix[mask & mask_up] = 2
    partition_matrix[mask & mask_down] = 3

    return partition_matrix


def csc_nce_torch(view1_feat, view2_feat, view1_origin, view2_origin, offset, match_index, nce_t, r1, r2, partitions=4):
    """masked_scene_contrast_v1m2_csc.py:212-254, statement for statement (the all-reduce is the model's)"""
    device = view1_feat.device
    loss = torch.tensor(0.0, device=device)
    pos_sim = torch.tensor(0.0, device=device)
    neg_sim = torch.tensor(0.0, device=device)
    large_num = 1e9

    view1_feat = view1_feat[match_index[:, 0]]
    view2_feat = view2_feat[match_index[:, 1]]
    view1_feat = view1_feat / (torch.norm(view1_feat, p=2, dim=1, keepdim=True) + 1e-7)
    view2_feat = view2_feat / (torch.norm(view2_feat, p=2, dim=1, keepdim=True) + 1e-7)

    view1_coord = view1_origin[match_index[:, 0]]
    view2_coord = view2_origin[match_index[:, 1]]

    batch = _offset2batch(offset, view1_origin.shape[0])[match_index[:, 0]]
    for batch_id in batch.unique():
        batch_mask = batch == batch_id
        sim = torch.mm(view1_feat[batch_mask], view2_feat[batch_mask].T)

        with torch.no_grad():
            pos_sim += torch.diagonal(sim).mean()
            neg_sim += sim.mean(dim=-1).mean() - pos_sim / batch_mask.sum()

        labels = torch.arange(sim.shape[0], device=view1_feat.device).long()
        part = compute_partitions_torch(view1_coord[batch_mask], view2_coord[batch_mask], r1, r2)
        for part_id in part.unique():
            part_mask = part == part_id
            part_mask.fill_diagonal_(True)
            loss = loss + torch.nn.functional.cross_entropy(
                torch.div(sim, nce_t) - large_num * (~part_mask).float(), labels, reduction="mean")

    loss = loss / (len(offset) * partitions)
    pos_sim /= len(offset)
    neg_sim /= len(offset)
    return loss, pos_sim, neg_sim


def group_pairs_by_scene(pairs, offset):
    """(pairs grouped by the scene of their view-1 row in a stable order, seg (b + 1) int32: the first row of every scene).
    Nothing is read back.  A view-1 index past the last scene end counts to the last scene (the kernels flag it)."""
    b = offset.numel()
    scene = torch.searchsorted(offset.long().contiguous(), pairs[:, 0].contiguous(), right=True).clamp_(max=b - 1)
    scene, order = torch.sort(scene, stable=True)
    seg = torch.searchsorted(scene, torch.arange(b + 1, device=pairs.device)).int()
    return pairs[order].contiguous(), seg.contiguous()


class _CscNCE(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, view1_feat, view2_feat, origin1, origin2, pairs, seg, nce_t, r1, r2, partitions):
        f1, f2 = view1_feat.contiguous(), view2_feat.contiguous()
        (n1, c), n2, m, b, dev = f1.shape, f2.shape[0], pairs.shape[0], seg.numel() - 1, f1.device
        L = _lib.lib()
        a = torch.empty((m, c), dtype=torch.float32, device=dev)
        bn = torch.empty((m, c), dtype=torch.float32, device=dev)
        norms = torch.empty((2, m), dtype=torch.float32, device=dev)
        coords = torch.empty((2, m, 3), dtype=torch.float32, device=dev)
        lse = torch.empty((CSC_CLASSES, m), dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _lib.workspace(L.ptv2_csc_nce_workspace_bytes(m, c, b), dev)
        rc = L.csc_nce_fwd_hip_launcher(n1, n2, m, c, b, f1.data_ptr(), f2.data_ptr(), origin1.data_ptr(), origin2.data_ptr(),
                                        pairs.data_ptr(), seg.data_ptr(), nce_t, r1, r2, partitions, a.data_ptr(), bn.data_ptr(),
                                        norms.data_ptr(), coords.data_ptr(), lse.data_ptr(), out.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "csc_nce_fwd_hip_launcher")  # (no read-back: a pair outside its operand turns the three outputs NaN)
        ctx.save_for_backward(pairs, seg, a, bn, norms, coords, lse)
        ctx.sizes = (n1, n2, nce_t, r1, r2, partitions)
        loss, pos_sim, neg_sim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(pos_sim, neg_sim)
        return loss, pos_sim, neg_sim

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_loss, g_pos, g_neg):
        pairs, seg, a, bn, norms, coords, lse = ctx.saved_tensors
        n1, n2, nce_t, r1, r2, partitions = ctx.sizes
        (m, c), b, dev = a.shape, seg.numel() - 1, a.device
        L = _lib.lib()
        # the order in which the rows of one index are summed: a stable sort of either column
        order = torch.stack([torch.sort(pairs[:, 0], stable=True)[1], torch.sort(pairs[:, 1], stable=True)[1]]).int().contiguous()
        g = g_loss.float().reshape(1).contiguous()
        df1 = torch.empty((n1, c), dtype=torch.float32, device=dev)
        df2 = torch.empty((n2, c), dtype=torch.float32, device=dev)
        ws = _lib.workspace(L.ptv2_csc_nce_workspace_bytes(m, c, b), dev)
        rc = L.csc_nce_bwd_hip_launcher(n1, n2, m, c, b, pairs.data_ptr(), seg.data_ptr(), order.data_ptr(), nce_t, r1, r2,
                                        partitions, a.data_ptr(), bn.data_ptr(), norms.data_ptr(), coords.data_ptr(),
                                        lse.data_ptr(), g.data_ptr(), df1.data_ptr(), df2.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr())
        _lib.check(rc, "csc_nce_bwd_hip_launcher")
        return df1, df2, None, None, None, None, None, None, None, None


def _csc_temperature_fits(nce_t):
    """1 / t <= CSC_MAX_INV_T as the launcher sees it, in fp32"""
    t = ctypes.c_float(nce_t).value
    return t > 0 and ctypes.c_float(1.0 / t).value <= CSC_MAX_INV_T


def csc_nce(view1_feat, view2_feat, view1_origin, view2_origin, offset, match_index, nce_t, r1, r2, partitions=4):
    """(loss, pos_sim, neg_sim) of masked_scene_contrast_v1m2_csc.py's compute_contrastive_loss on one rank, in fp32 (under
    autocast too).  view1_feat (n1, C), view2_feat (n2, C), view1_origin (n1, 3), view2_origin (n2, 3), offset (B) the ascending
    scene ends of view 1, match_index (M, 2).  A pair belongs to the scene of its view-1 row.  Inside a scene, with a_i, b_j the
    rows the pairs name, each divided by its norm + 1e-7, S_ij = a_i.b_j, and class(i, j) one of none, 0, 1, 2, 3 from
    rel = view1_origin[match[j, 0]] - view2_origin[match[i, 1]]:

        loss = sum_scenes sum_classes mean_i(logsumexp_{j: class(i, j) = k or j = i}(S_ij / t) - S_ii / t) / (B partitions)

    pos_sim and neg_sim follow the reference's scene recurrences, both divided by B.  Only the loss carries a gradient.
    1 <= M <= CSC_MAX_PAIRS, C a multiple of 4 up to CSC_MAX_CHANNELS, B <= CSC_MAX_SCENES and 1 / t <= CSC_MAX_INV_T run on
    the tiled kernels, which never hold an (M, M) array; anything else takes the eager statements.  M = 0 raises (the reference
    returns zeros).  A pair that names a row outside its operand makes the three outputs NaN on the kernels (nothing is read
    back to raise on) and contributes no gradient."""
    _lib.require_cuda(view1_feat, view2_feat, view1_origin, view2_origin, offset, match_index)
    if view1_feat.dim() != 2 or view2_feat.dim() != 2 or view1_feat.shape[1] != view2_feat.shape[1] or match_index.dim() != 2 \
            or match_index.shape[1] != 2 or match_index.is_floating_point() or tuple(view1_origin.shape) != (view1_feat.shape[0], 3) \
            or tuple(view2_origin.shape) != (view2_feat.shape[0], 3) or offset.dim() != 1 or offset.numel() < 1:
        raise ValueError("ao_amd msc: csc_nce takes (n1, C), (n2, C), (n1, 3), (n2, 3), (B) and integer (M, 2); got %s %s %s %s %s %s %s" % (
            tuple(view1_feat.shape), tuple(view2_feat.shape), tuple(view1_origin.shape), tuple(view2_origin.shape),
            tuple(offset.shape), tuple(match_index.shape), match_index.dtype))
    m, c, b = match_index.shape[0], view1_feat.shape[1], offset.numel()
    if m == 0:
        raise ValueError("ao_amd msc: csc_nce of no pair (the loss is a mean over the pairs of a scene)")
    if not float(nce_t) > 0:
        raise ValueError("ao_amd msc: nce_t %r (> 0)" % (nce_t,))
    if int(partitions) < 1:
        raise ValueError("ao_amd msc: partitions %r (>= 1)" % (partitions,))
    pairs = match_index.long().contiguous()
    origin1, origin2 = view1_origin.detach().float().contiguous(), view2_origin.detach().float().contiguous()
    fits = m <= CSC_MAX_PAIRS and 4 <= c <= CSC_MAX_CHANNELS and c % 4 == 0 and view1_feat.shape[0] > 0 and view2_feat.shape[0] > 0 \
        and b <= CSC_MAX_SCENES and _csc_temperature_fits(float(nce_t))
    if not use_hip() or not fits:
        with torch.autocast("cuda", enabled=False):
            return csc_nce_torch(view1_feat.float(), view2_feat.float(), origin1, origin2, offset, pairs, float(nce_t), float(r1),
                                 float(r2), int(partitions))
    pairs, seg = group_pairs_by_scene(pairs, offset)
    return _CscNCE.apply(view1_feat, view2_feat, origin1, origin2, pairs, seg, float(nce_t), float(r1), float(r2), int(partitions))


# --------------------------------------------------------------------------------------------------------- matching ----
def _match_torch(idx, dist2, row_draws, max_k, max_radius):
    """:154-169 with the draw of a matched row taken from row_draws"""
    distance = torch.sqrt(dist2)
    index = torch.cat([torch.arange(idx.shape[0], device=idx.device, dtype=torch.long).view(-1, 1, 1).expand(-1, max_k, 1),
                       idx.long().view(-1, max_k, 1)], dim=-1)[(distance < max_radius) & (idx >= 0)]
    if index.shape[0] == 0:
        return index.view(0, 2)
    unique, count = index[:, 0].unique(return_counts=True)
    select = torch.cumsum(count, dim=0) - row_draws[unique] % count - 1
    return index[select]


@torch.no_grad()
def match_pairs(coord1, offset1, coord2, offset2, max_k, max_radius, max_pair, row_draws=None, perm=None, generator=None):
    """match_index (M, 2) int64 of :147-172: for every view-1 point with a view-2 point of the same scene among its max_k
    nearest at a distance (fp32, square-rooted) below max_radius, one of those, in ascending view-1 order; cut to max_pair rows
    through a permutation when there are more.

    row_draws (n1) int64: the reference's draw of each row (it draws one per matched row, below the largest hit count); a
    negative draw reads as 0.  None draws them on the device, uniformly below 2^31, so that every hit of a row is equally
    likely (the reference's `randint(count.max()) % count` favours the later hits of a row with fewer hits than the largest).
    perm (P): the permutation of the P matched rows, used when P > max_pair; None draws it then.  generator: a torch.Generator
    of the coordinates' device for the draws.  One read-back: the number of matched rows."""
    _lib.require_cuda(coord1, offset1, coord2, offset2)
    if coord1.dim() != 2 or coord1.shape[1] != 3 or coord2.dim() != 2 or coord2.shape[1] != 3 or offset1.shape != offset2.shape:
        raise ValueError("ao_amd msc: match_pairs takes (n1, 3), (b), (n2, 3), (b); got %s %s %s %s" % (
            tuple(coord1.shape), tuple(offset1.shape), tuple(coord2.shape), tuple(offset2.shape)))
    max_k = int(max_k)
    if not 1 <= max_k <= MAX_K:
        raise ValueError("ao_amd msc: max_k %d (1..%d)" % (max_k, MAX_K))
    dev, n1, n2 = coord1.device, coord1.shape[0], coord2.shape[0]
    if n1 == 0 or n2 == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=dev)
    idx, dist2 = knn_query_dist2(max_k, coord2.float().contiguous(), offset2.int(), coord1.float().contiguous(), offset1.int())
    if row_draws is None:
        row_draws = torch.randint(0, 1 << 31, (n1,), device=dev, generator=generator)
    row_draws = row_draws.to(dev).long().contiguous()
    if row_draws.shape != (n1,):
        raise ValueError("ao_amd msc: row_draws %s for %d view-1 points" % (tuple(row_draws.shape), n1))
    if use_hip():
        chosen = torch.empty(n1, dtype=torch.int64, device=dev)
        rc = _lib.lib().msc_match_hip_launcher(n1, max_k, n2, idx.data_ptr(), dist2.data_ptr(), row_draws.data_ptr(),
                                               float(max_radius), chosen.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "msc_match_hip_launcher")
        rows = (chosen >= 0).nonzero().view(-1)  # THE read-back: the number of pairs
        index = torch.stack([rows, chosen[rows]], 1)
    else:
        index = _match_torch(idx, dist2, row_draws.clamp(min=0), max_k, max_radius)
    p = index.shape[0]
    if p > max_pair:
        if perm is None:
            perm = torch.randperm(p, generator=generator, device=dev if generator is None else generator.device)
        if perm.numel() != p:
            raise ValueError("ao_amd msc: perm of %d entries for %d matched rows" % (perm.numel(), p))
        index = index[perm[:max_pair].to(dev).long()]
    return index


# ------------------------------------------------------------------------------------------------------ cross masks ----
def _grid_tensor(mask_grid_size, device):
    """the divisor as a one-element fp32 tensor: torch divides by a python scalar through its rounded reciprocal on the GPU"""
    return torch.full((1,), float(mask_grid_size), dtype=torch.float32, device=device)


def _patch_ids_torch(origin1, offset1, origin2, offset2, mask_grid_size):
    """:94-98 over the points of view 1, then of view 2 (the ids do not depend on the order of the union), voxel_grid written
    out: id = sum_d trunc(p_d) prod_{e<d} (trunc(max_e) + 1) over p = (cell, scene)"""
    cell = torch.floor(torch.cat([origin1, origin2]).div(_grid_tensor(mask_grid_size, origin1.device)))
    batch = torch.cat([_offset2batch(offset1, origin1.shape[0]), _offset2batch(offset2, origin2.shape[0])])
    p = torch.cat([cell, batch.view(-1, 1).to(cell.dtype)], dim=-1)
    num = p.max(0)[0].long() + 1
    num = torch.cat([num.new_ones(1), num.cumprod(0)])[:4]
    return (p.long() * num.view(1, -1)).sum(1)


def patch_ids(origin1, offset1, origin2, offset2, mask_grid_size):
    """int64 (n1 + n2): the cluster id of voxel_grid(pos=floor(origin / mask_grid_size), size=1, batch=scene, start=0) for the
    points of view 1, then of view 2, the maxima taken over both.  Cells are not shifted to zero: a negative cell can carry the
    id of another cell, as in the reference."""
    _lib.require_cuda(origin1, offset1, origin2, offset2)
    if origin1.dim() != 2 or origin1.shape[1] != 3 or origin2.dim() != 2 or origin2.shape[1] != 3 or offset1.dim() != 1 \
            or offset1.shape != offset2.shape or offset1.numel() < 1 or origin1.shape[0] + origin2.shape[0] == 0 \
            or not float(mask_grid_size) > 0:
        raise ValueError("ao_amd msc: patch ids of (n1, 3), (b), (n2, 3), (b) with n1 + n2 >= 1, b >= 1 and a positive grid; got "
                         "%s %s %s %s, grid %r" % (tuple(origin1.shape), tuple(offset1.shape), tuple(origin2.shape),
                                                   tuple(offset2.shape), mask_grid_size))
    n1, n2, dev = origin1.shape[0], origin2.shape[0], origin1.device
    origin1, origin2 = origin1.float().contiguous(), origin2.float().contiguous()
    if not use_hip():
        return _patch_ids_torch(origin1, offset1, origin2, offset2, mask_grid_size)
    # floor and the division are monotone: the largest cell is the cell of the largest coordinate
    top = origin1.amax(0) if n2 == 0 else origin2.amax(0) if n1 == 0 else torch.maximum(origin1.amax(0), origin2.amax(0))
    cell_max = torch.floor(top.div(_grid_tensor(mask_grid_size, dev))).contiguous()
    ids = torch.empty(n1 + n2, dtype=torch.int64, device=dev)
    off1, off2 = offset1.int().contiguous(), offset2.int().contiguous()
    rc = _lib.lib().msc_patch_ids_hip_launcher(n1, n2, off1.numel(), origin1.data_ptr(), off1.data_ptr(), origin2.data_ptr(),
                                               off2.data_ptr(), float(mask_grid_size), cell_max.data_ptr(), ids.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "msc_patch_ids_hip_launcher")
    return ids


@torch.no_grad()
def cross_masks(origin1, offset1, origin2, offset2, mask_grid_size, mask_rate, perm=None, generator=None):
    """(view1_point_mask (n1) bool, view2_point_mask (n2) bool) of :94-141: the patches of the union of both views, numbered by
    ascending id; with m = int(patch_num * mask_rate), the patches perm[:m] are masked in view 1 and perm[m:2m] in view 2.
    perm (patch_num): None draws torch.randperm(patch_num, generator=generator)."""
    if mask_rate > 0.5:
        raise ValueError("ao_amd msc: mask_rate %r (at most 0.5: the two views mask disjoint patches)" % (mask_rate,))
    _lib.require_cuda(origin1, offset1, origin2, offset2)
    if origin1.dim() != 2 or origin2.dim() != 2:
        raise ValueError("ao_amd msc: cross_masks takes (n1, 3), (b), (n2, 3), (b); got %s %s" % (tuple(origin1.shape), tuple(origin2.shape)))
    n1, n2, dev = origin1.shape[0], origin2.shape[0], origin1.device
    mask1 = torch.zeros(n1, dtype=torch.bool, device=dev)
    mask2 = torch.zeros(n2, dtype=torch.bool, device=dev)
    if mask_rate == 0 or n1 + n2 == 0:
        return mask1, mask2
    ids = patch_ids(origin1, offset1, origin2, offset2, mask_grid_size)
    unique, cluster = torch.unique(ids, sorted=True, return_inverse=True)
    patch_num = unique.shape[0]
    m = int(patch_num * mask_rate)
    if perm is None:
        perm = torch.randperm(patch_num, generator=generator, device="cpu" if generator is None else generator.device)
    if perm.numel() != patch_num:
        raise ValueError("ao_amd msc: perm of %d entries for %d patches" % (perm.numel(), patch_num))
    perm = perm.to(dev).long()
    tag = torch.zeros(patch_num, dtype=torch.int32, device=dev)
    tag[perm[0:m]] = 1
    tag[perm[m:m * 2]] = 2
    point_tag = tag[cluster]
    return point_tag[:n1] == 1, point_tag[n1:] == 2
