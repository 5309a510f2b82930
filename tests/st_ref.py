"""Plain-torch restatements of what ao_amd.stratified computes, for any floating dtype and any device.

Continuous quantities follow the dtype of their inputs.  Integer quantities -- the window cells and the relative-position index --
are ALWAYS computed in fp32 from fp32 coordinates, as the model does: in float64 a coordinate on a cell edge rounds to the other
side and another table row is read, which is a different function and not a more exact one.

Line numbers: pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py of the reference.
torch_geometric.voxel_grid, torch_scatter.scatter_softmax, torch_points_kernels.ball_query and torch_points3d's KPConvLayer are
restated from their published definitions; none of these libraries is available to check against.
"""
import math

import torch


# ---------------------------------------------------------------------------------------------------------- cells ----
def offset2batch(offset, n):
    return torch.searchsorted(offset.long().to(offset.device), torch.arange(n, device=offset.device), right=True)


def voxel_cells(pos, size, start):
    """voxel_grid's cell per axis: trunc((pos - start) / size), fp32 (only the partition it induces matters)"""
    return torch.div(pos.float() - start.float(), size.float(), rounding_mode="trunc").long()


def cluster_ids(cell, batch):
    """consecutive ids 0..V-1 of the distinct (cell, cloud) rows, as torch.unique(..., return_inverse=True) numbers them"""
    rows = torch.cat([cell, batch.view(-1, 1)], 1)
    return torch.unique(rows, dim=0, sorted=True, return_inverse=True)[1]


def grid_sample(coords, batch, size, start):
    """:40-57: (cluster, p2v_map, counts)"""
    if start is None:
        start = coords.min(0).values
    cluster = cluster_ids(voxel_cells(coords, size, start), batch)
    unique, cluster, counts = torch.unique(cluster, sorted=True, return_inverse=True, return_counts=True)
    n, k = unique.shape[0], int(counts.max())
    p2v_map = cluster.new_zeros(n, k)
    mask = torch.arange(k, device=coords.device).unsqueeze(0) < counts.unsqueeze(-1)
    p2v_map[mask] = torch.argsort(cluster, stable=True)
    return cluster, p2v_map, counts


def pair_lists(coords, offset, down_idx, window_size, shifted):
    """:331-417 for one block: (index_0, index_1) int64, rows sorted by (index_0, index_1); the mask statements as they stand."""
    coords = coords.float()
    dev = coords.device
    window = torch.tensor([window_size] * 3, dtype=coords.dtype, device=dev)
    new_window = 2 * torch.tensor([window_size] * 3, dtype=coords.dtype, device=dev)
    batch = offset2batch(offset, coords.shape[0])
    coords_min = coords.min(0).values
    if not shifted:
        _, p2v_map_blk, counts_blk = grid_sample(coords, batch, window, None)
        _, new_p2v_map_blk, new_counts_blk = grid_sample(coords, batch, new_window, None)
    else:
        shift_size = window * 1 / 2
        _, p2v_map_blk, counts_blk = grid_sample(coords + shift_size, batch, window, coords_min)
        shift_size = new_window * 1 / 2
        _, new_p2v_map_blk, new_counts_blk = grid_sample(coords + shift_size, batch, new_window, coords_min)

    n, k = p2v_map_blk.shape
    mask = torch.arange(k, device=dev).unsqueeze(0) < counts_blk.unsqueeze(-1)
    mask_mat = mask.unsqueeze(-1) & mask.unsqueeze(-2)
    index_0 = p2v_map_blk.unsqueeze(-1).expand(-1, -1, k)[mask_mat]
    index_1 = p2v_map_blk.unsqueeze(1).expand(-1, k, -1)[mask_mat]

    down_mask = torch.zeros_like(batch).bool()
    down_mask[down_idx.long()] = True
    down_mask = down_mask[new_p2v_map_blk]
    n, k = new_p2v_map_blk.shape
    mask = torch.arange(k, device=dev).unsqueeze(0) < new_counts_blk.unsqueeze(-1)
    down_mask = down_mask & mask
    mask_mat = mask.unsqueeze(-1) & down_mask.unsqueeze(-2)
    if not shifted:
        window_coord = torch.div(coords[new_p2v_map_blk] - coords_min, window, rounding_mode="trunc")
    else:
        window_coord = torch.div(coords[new_p2v_map_blk] - coords_min + 1 / 2 * window, window, rounding_mode="trunc")
    mask_mat_prev = (window_coord.unsqueeze(2) != window_coord.unsqueeze(1)).any(-1)
    mask_mat = mask_mat & mask_mat_prev
    new_index_0 = new_p2v_map_blk.unsqueeze(-1).expand(-1, -1, k)[mask_mat]
    new_index_1 = new_p2v_map_blk.unsqueeze(1).expand(-1, k, -1)[mask_mat]
    index_0 = torch.cat([index_0, new_index_0], 0)
    index_1 = torch.cat([index_1, new_index_1], 0)
    order = torch.argsort(index_0 * coords.shape[0] + index_1)
    return index_0[order], index_1[order]


def csr_of(index_0, n):
    counts = torch.bincount(index_0, minlength=n)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]), int(counts.max())


def cells_eager(coords, start, window_size, shifted):
    """(grid cell, window coordinate :394-406) of every point, int64 (N, 3), by the eager fp32 statements"""
    coords = coords.float()
    window = torch.tensor([window_size] * 3, dtype=coords.dtype, device=coords.device)
    if not shifted:
        return voxel_cells(coords, window, start), torch.div(coords - start, window, rounding_mode="trunc").long()
    return (voxel_cells(coords + window * 1 / 2, window, start),
            torch.div(coords - start + 1 / 2 * window, window, rounding_mode="trunc").long())


# ------------------------------------------------------------------------------------------------- relative index ----
def quant_grid_length(window_size, quant_size):
    return int((2 * window_size + 1e-4) // quant_size)


def rel_index(coords, index_0, index_1, window_size, quant_size):
    """:145-151 in fp32: (M, 3) int64, and whether the asserts of :153-154 hold"""
    coords = coords.float()
    relative_position = coords[index_0] - coords[index_1]
    relative_position = torch.round(relative_position * 100000) / 100000
    relative_position_index = torch.div(relative_position + 2 * window_size - 1e-4, quant_size, rounding_mode="trunc")
    ok = bool((relative_position_index >= 0).all()) and \
        bool((relative_position_index <= 2 * quant_grid_length(window_size, quant_size) - 1).all())
    return relative_position_index.long(), ok


# ------------------------------------------------------------------------------------------- the three operators ----
def _lookup(table, rel):
    """(M, h, hdim): the three axes' rows of a (L, h, hdim, 3) table, summed (rpe_v2: table[r0, .., 0] + [r1, .., 1] + [r2, .., 2])"""
    return table[rel[:, 0], :, :, 0] + table[rel[:, 1], :, :, 1] + table[rel[:, 2], :, :, 2]


def attention_step1(q, k, index_0, index_1):
    return (q[index_0] * k[index_1]).sum(-1)


def dot_prod_with_idx(q, k, index_0, index_1, table_q, table_k, rel):
    return (q[index_0] * _lookup(table_q, rel)).sum(-1) + (k[index_1] * _lookup(table_k, rel)).sum(-1)


def scatter_softmax(src, index_0, n):
    with torch.no_grad():
        top = torch.full((n,) + src.shape[1:], float("-inf"), dtype=src.dtype, device=src.device)
        top = top.scatter_reduce(0, index_0.view(-1, 1).expand_as(src), src, "amax")
    e = torch.exp(src - top[index_0])
    return e / torch.zeros_like(top).index_add_(0, index_0, e)[index_0]


def attention_step2(attn, v, index_0, index_1, table, rel):
    out = torch.zeros_like(v)
    return out.index_add_(0, index_0, attn.unsqueeze(-1) * (v[index_1] + _lookup(table, rel)))


def window_attention(q, k, v, coords, index_0, index_1, table_q, table_k, table_v, window_size, quant_size):
    """WindowAttention.forward :140-202 between the qkv projection and the output projection; q already scaled"""
    n, h, hd = q.shape
    rel, _ = rel_index(coords, index_0, index_1, window_size, quant_size)
    attn = attention_step1(q, k, index_0, index_1) + dot_prod_with_idx(q, k, index_0, index_1, table_q, table_k, rel)
    p = scatter_softmax(attn, index_0, n)
    return attention_step2(p, v, index_0, index_1, table_v, rel).view(n, h * hd)


# ------------------------------------------------------------------------------------------------------ the stem ----
def ball_query(radius, max_n, x, batch):
    """tp.ball_query(radius, max_n, x, x, mode="partial_dense", batch_x=batch, batch_y=batch)[0]: (N, max_n) int64, per point the
    max_n smallest indices j of its own cloud with |x_j - x_i|^2 < radius^2 (itself included), unused slots N"""
    n = x.shape[0]
    xf = x.float()
    d2 = ((xf.unsqueeze(1) - xf.unsqueeze(0)) ** 2).sum(-1)
    hit = (d2 < radius * radius) & (batch.view(-1, 1) == batch.view(1, -1))
    j = torch.arange(n, device=x.device).view(1, -1).expand(n, -1)
    ranked = torch.where(hit, j, torch.full_like(j, n)).sort(1)[0]
    if ranked.shape[1] < max_n:
        ranked = torch.cat([ranked, ranked.new_full((n, max_n - ranked.shape[1]), n)], 1)
    return ranked[:, :max_n].contiguous()


def kernel_points(point_influence, dtype=torch.float32):
    """the deterministic disposition ao_amd uses in place of the library's optimised one: the centre, the six axis points and
    the eight cube corners, each at 2/3 of the radius 1.5 * point_influence"""
    r = 1.5 * point_influence * 2.0 / 3.0
    pts = [(0.0, 0.0, 0.0)]
    for a in range(3):
        for s in (1.0, -1.0):
            p = [0.0, 0.0, 0.0]
            p[a] = s
            pts.append(tuple(p))
    c = 1.0 / math.sqrt(3.0)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                pts.append((sx * c, sy * c, sz * c))
    return torch.tensor(pts, dtype=torch.float64).mul(r).to(dtype)


def kpconv(xyz, neighbor_idx, feats, weight, k_points, kp_extent):
    """KPConvLayer.forward(xyz, xyz, neighbor_idx, feats), linear influence, sum aggregation, add_one=False:
    out_i = sum_k (sum_m max(0, 1 - |x_nbr(i,m) - x_i - K_k| / extent) f_nbr(i,m)) @ weight[k]; a shadow neighbour (index N)
    lies far away and carries zero features"""
    n = xyz.shape[0]
    pad = torch.cat([xyz, torch.full_like(xyz[:1], 1e6)], 0)
    fpad = torch.cat([feats, torch.zeros_like(feats[:1])], 0)
    rel = pad[neighbor_idx] - xyz.unsqueeze(1)                                  # (N, m, 3)
    dist = (rel.unsqueeze(2) - k_points.view(1, 1, -1, 3)).pow(2).sum(-1).sqrt()  # (N, m, K)
    infl = torch.clamp(1 - dist / kp_extent, min=0.0)
    infl = infl * (neighbor_idx < n).unsqueeze(-1).to(infl.dtype)
    weighted = torch.matmul(infl.transpose(1, 2), fpad[neighbor_idx])           # (N, K, cin)
    return torch.einsum("nkc,kcd->nd", weighted, weight)
