"""The stem of Stratified Transformer: ball query, KPConv and FastBatchNorm1d (ao_amd/csrc/kpconv.hip).

torch_points_kernels and torch_points3d are not available to this project: `ball_query` and `KPConvLayer` restate the published
definitions of `tp.ball_query(..., mode="partial_dense")` and of KPConvLayer with linear influence and sum aggregation, and have
not been run against those libraries.  The library loads optimised kernel-point dispositions from disk; `kernel_points` is a
deterministic stand-in.  `K_points` is in the state dict, so a checkpoint of the reference overwrites it.

AO_AMD_ST=torch runs the eager statements instead of the kernels.
"""
import math

import torch
import torch.nn as nn

from .. import _abi, _lib
from ..pointgroup.ops import ball_query as _ball_query_csr
from . import ops

KP_POINTS = _abi.st_consts["ST_KP_POINTS"]


@torch.no_grad()
def ball_query(radius, max_n, x, offset):
    """tp.ball_query(radius, max_n, x, x, mode="partial_dense", batch_x=batch, batch_y=batch)[0]: (N, max_n) int64, per point the
    max_n smallest indices j of its own cloud with |x_j - x_i|^2 < radius^2 (itself included); unused slots hold N, the shadow
    row.  offset (b): the ascending cloud ends."""
    _lib.require_cuda(x, offset)
    n, dev = x.shape[0], x.device
    starts = torch.cat([offset.new_zeros(1), offset]).int()
    idx, start_len, _ = _ball_query_csr(x.float().contiguous(), starts, radius)   # ascending lists, capped far above any max_n
    slot = torch.arange(int(max_n), device=dev).view(1, -1)
    start, length = start_len[:, 0].long().view(-1, 1), start_len[:, 1].long().view(-1, 1)
    have = slot < length
    at = torch.where(have, start + slot, torch.zeros_like(slot))
    if idx.numel() == 0:
        return torch.full((n, int(max_n)), n, dtype=torch.int64, device=dev)
    return torch.where(have, idx.long()[at], torch.full_like(at, n)).contiguous()


def kernel_points(point_influence):
    """(15, 3): the centre, the six axis points and the eight cube corners, each at 2/3 of the radius 1.5 * point_influence"""
    r = 1.5 * point_influence * 2.0 / 3.0
    pts = [(0.0, 0.0, 0.0)]
    for a in range(3):
        for s in (1.0, -1.0):
            p = [0.0, 0.0, 0.0]
            p[a] = s
            pts.append(tuple(p))
    c = 1.0 / math.sqrt(3.0)
    pts += [(sx * c, sy * c, sz * c) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    return torch.tensor(pts, dtype=torch.float64).mul(r).float()


def transpose_neighbors(neighbor_idx, n):
    """(t_offsets (N + 1) int32, t_src (slots) int32): for every point j the points i whose row holds j, once per slot,
    ascending by (i, slot)"""
    flat = neighbor_idx.reshape(-1)
    live = (flat >= 0) & (flat < n)
    src = torch.arange(neighbor_idx.shape[0], device=flat.device).repeat_interleave(neighbor_idx.shape[1])[live]
    key = flat[live]
    order = torch.sort(key, stable=True)[1]
    counts = torch.bincount(key, minlength=n)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int().contiguous(), src[order].int().contiguous()


def weighted_features_torch(xyz, neighbor_idx, feats, k_points, extent):
    """(N, 15 * cin) by eager statements"""
    n = xyz.shape[0]
    pad = torch.cat([xyz, torch.full_like(xyz[:1], 1e6)], 0)
    fpad = torch.cat([feats, torch.zeros_like(feats[:1])], 0)
    nbr = torch.where((neighbor_idx >= 0) & (neighbor_idx < n), neighbor_idx, torch.full_like(neighbor_idx, n))
    rel = pad[nbr] - xyz.unsqueeze(1)
    dist = (rel.unsqueeze(2) - k_points.view(1, 1, -1, 3)).pow(2).sum(-1).sqrt()
    infl = torch.clamp(1 - dist / extent, min=0.0) * (nbr < n).unsqueeze(-1).to(feats.dtype)
    return torch.matmul(infl.transpose(1, 2), fpad[nbr]).reshape(n, -1)


class _WeightedFeatures(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, feats, xyz, neighbor_idx, k_points, extent):
        feats, xyz, nbr, kp = feats.contiguous(), xyz.contiguous(), neighbor_idx.contiguous(), k_points.contiguous()
        (n, cin), max_n = feats.shape, nbr.shape[1]
        out = torch.empty((n, KP_POINTS * cin), dtype=torch.float32, device=feats.device)
        rc = _lib.lib().st_kpconv_fwd_hip_launcher(n, max_n, cin, xyz.data_ptr(), nbr.data_ptr(), feats.data_ptr(), kp.data_ptr(),
                                                   extent, out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "st_kpconv_fwd_hip_launcher")
        # the transposed neighbour lists of the backward, made once per forward
        t_offsets, t_src = transpose_neighbors(nbr, n) if ctx.needs_input_grad[0] else (None, None)
        ctx.save_for_backward(xyz, kp, t_offsets, t_src)
        ctx.sizes = (n, cin, extent)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        xyz, kp, t_offsets, t_src = ctx.saved_tensors
        n, cin, extent = ctx.sizes
        g = g.contiguous()
        g_feats = torch.empty((n, cin), dtype=torch.float32, device=g.device)
        rc = _lib.lib().st_kpconv_bwd_hip_launcher(n, cin, t_src.numel(), xyz.data_ptr(), t_offsets.data_ptr(), _lib.ptr(t_src),
                                                   kp.data_ptr(), extent, g.data_ptr(), g_feats.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "st_kpconv_bwd_hip_launcher")
        return g_feats, None, None, None, None


def weighted_features(xyz, neighbor_idx, feats, k_points, extent):
    """(N, 15 * cin): per point and kernel point the influence-weighted sum of the neighbours' features.  No gradient reaches
    the coordinates or the kernel points."""
    _lib.require_cuda(xyz, neighbor_idx, feats, k_points)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or feats.dim() != 2 or feats.shape[0] != xyz.shape[0] or neighbor_idx.dim() != 2 \
            or neighbor_idx.shape[0] != xyz.shape[0] or neighbor_idx.dtype != torch.int64 or k_points.shape != (KP_POINTS, 3):
        raise ValueError("ao_amd stratified: KPConv takes xyz (N, 3), int64 neighbor_idx (N, max_n), feats (N, cin), K_points (15, 3); "
                         "got %s %s %s %s %s" % (tuple(xyz.shape), tuple(neighbor_idx.shape), neighbor_idx.dtype, tuple(feats.shape),
                                                 tuple(k_points.shape)))
    if ops.mode() == "torch":
        with torch.autocast("cuda", enabled=False):
            return weighted_features_torch(xyz.float(), neighbor_idx, feats.float(), k_points.float(), float(extent))
    return _WeightedFeatures.apply(feats, xyz.float(), neighbor_idx, k_points.float(), float(extent))


class KPConvLayer(nn.Module):
    """KPConvLayer(cin, cout, point_influence, add_one=False) of torch_points3d: 15 kernel points, linear influence with
    KP_extent = point_influence, sum aggregation.  `weight` (15, cin, cout) xavier-normal; `K_points` (15, 3) a parameter without
    gradient, initialised by kernel_points()."""

    def __init__(self, num_inputs, num_outputs, point_influence, add_one=False):
        super().__init__()
        if add_one:
            raise NotImplementedError("ao_amd stratified: KPConvLayer(add_one=True) is not provided (ST-v1m2 passes False)")
        self.num_inputs, self.num_outputs, self.KP_extent = num_inputs, num_outputs, point_influence
        self.K_points = nn.Parameter(kernel_points(point_influence), requires_grad=False)
        self.weight = nn.Parameter(torch.empty(KP_POINTS, num_inputs, num_outputs))
        nn.init.xavier_normal_(self.weight)

    def forward(self, query_points, support_points, neighbors, x):
        if query_points is not support_points and not torch.equal(query_points, support_points):
            raise NotImplementedError("ao_amd stratified: KPConvLayer with query points other than the support points")
        weighted = weighted_features(support_points, neighbors, x, self.K_points, self.KP_extent)
        with torch.autocast("cuda", enabled=False):
            return torch.matmul(weighted, self.weight.float().reshape(KP_POINTS * self.num_inputs, self.num_outputs))


class FastBatchNorm1d(nn.Module):
    """torch_points3d's wrapper: keys `...batch_norm.weight`"""

    def __init__(self, num_features, momentum=0.1, **kwargs):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(num_features, momentum=momentum, **kwargs)

    def forward(self, x):
        return self.batch_norm(x)
