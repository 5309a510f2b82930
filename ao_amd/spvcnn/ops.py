"""SPVCNN's two point-voxel operators on ao_amd/csrc/spv_ops.hip (C ABI include/ptv2_spv_hip.h), each one
autograd node over a PointVoxelMap.

    devoxelize(feat, pvmap, level, add=None)   voxel_to_point: out[i] = sum_j (w_j / W) feat[corner_j(i)] (+ add[i]), the trilinear
                                               weights of calc_ti_weights over the eight cell corners, formed in registers
    voxelize(feat, pvmap, level)               initial_voxelize / point_to_voxel: the mean of the point rows of each voxel

The forward of devoxelize keeps one float per point (W); no (n, 8) tensor exists and no sum uses an atomic.

AO_AMD_SPVCNN (read on every call): unset or "hip": the kernels; "torch": the same statements as eager torch on the same map
(gathers over an explicit (n, 8) table, index_add), in the dtype of `feat`.  There is no CPU fallback on either path.
"""
import os

import torch

from .. import _abi, _lib
from .pvmap import LEVELS, PointVoxelMap

MAX_CHANNELS, SMALL_CHANNELS = _abi.spv_consts["SPV_MAX_CHANNELS"], _abi.spv_consts["SPV_SMALL_CHANNELS"]
# corner j = 4 jx + 2 jy + jz of a cell is column 9 (jx + 1) + 3 (jy + 1) + (jz + 1) of the k = 3 table
CORNER_COLUMNS = tuple(13 + 9 * (j >> 2) + 3 * ((j >> 1) & 1) + (j & 1) for j in range(8))


def mode():
    m = os.environ.get("AO_AMD_SPVCNN", "hip")
    if m not in ("hip", "torch"):
        raise ValueError("ao_amd spvcnn: AO_AMD_SPVCNN=%r (hip or torch)" % m)
    return m


# ------------------------------------------------------------------------------------------------------- eager torch -------
def corner_table(pvmap, level, dtype=torch.float32):
    """The (n, 8) corner rows (-1: no voxel) and normalised weights that the HIP path never forms"""
    cols = torch.tensor(CORNER_COLUMNS, device=pvmap.coord.device)
    idx = pvmap.tables.nbr3[level].index_select(0, pvmap.row[level].long()).index_select(1, cols)
    f = (pvmap.coord & ((1 << level) - 1)).to(dtype) / (1 << level)
    w = torch.ones((pvmap.n, 8), dtype=dtype, device=f.device)
    for j in range(8):
        for a in range(3):
            w[:, j] *= f[:, a] if (j >> (2 - a)) & 1 else 1 - f[:, a]
    w = w * (idx >= 0).to(dtype)
    return idx, w / (w.sum(1, keepdim=True) + 1e-8)


def devoxelize_torch(feat, pvmap, level, add=None):
    idx, w = corner_table(pvmap, level, feat.dtype)
    out = (feat.index_select(0, idx.clamp(min=0).reshape(-1).long()).view(pvmap.n, 8, -1) * w.unsqueeze(2)).sum(1)
    return out if add is None else out + add


def voxelize_torch(feat, pvmap, level):
    total = feat.new_zeros((pvmap.n_vox[level], feat.shape[1])).index_add(0, pvmap.row[level].long(), feat)
    return total / pvmap.counts(level).to(feat.dtype).unsqueeze(1)


# --------------------------------------------------------------------------------------------------------------- HIP -------
class _Devoxelize(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, feat, add, pvmap, level):
        feat = feat.contiguous()
        add = None if add is None else add.contiguous()
        n, c = pvmap.n, feat.shape[1]
        out = torch.empty((n, c), dtype=torch.float32, device=feat.device)
        wsum = torch.empty(n, dtype=torch.float32, device=feat.device)
        rc = _lib.lib().spv_devoxelize_fwd_hip_launcher(n, feat.shape[0], c, level, pvmap.coord.data_ptr(), pvmap.row[level].data_ptr(),
                                                        pvmap.tables.nbr3[level].data_ptr(), feat.data_ptr(), _lib.ptr(add),
                                                        out.data_ptr(), wsum.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "spv_devoxelize_fwd_hip_launcher")
        ctx.save_for_backward(wsum)
        ctx.pvmap, ctx.level, ctx.n_vox = pvmap, level, feat.shape[0]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        (wsum,), pvmap, level = ctx.saved_tensors, ctx.pvmap, ctx.level
        g = g.contiguous()
        g_feat = None
        if ctx.needs_input_grad[0]:
            g_feat = torch.empty((ctx.n_vox, g.shape[1]), dtype=torch.float32, device=g.device)
            rc = _lib.lib().spv_devoxelize_bwd_hip_launcher(pvmap.n, ctx.n_vox, g.shape[1], level, pvmap.coord.data_ptr(),
                                                            pvmap.tables.nbr3[level].data_ptr(), pvmap.start[level].data_ptr(),
                                                            pvmap.order[level].data_ptr(), wsum.data_ptr(), g.data_ptr(),
                                                            g_feat.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "spv_devoxelize_bwd_hip_launcher")
        return g_feat, (g if ctx.needs_input_grad[1] else None), None, None


class _Voxelize(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, feat, pvmap, level):
        feat = feat.contiguous()
        n_vox, c = pvmap.n_vox[level], feat.shape[1]
        out = torch.empty((n_vox, c), dtype=torch.float32, device=feat.device)
        rc = _lib.lib().spv_voxelize_fwd_hip_launcher(pvmap.n, n_vox, c, level, pvmap.start[level].data_ptr(),
                                                      pvmap.order[level].data_ptr(), feat.data_ptr(), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "spv_voxelize_fwd_hip_launcher")
        ctx.pvmap, ctx.level = pvmap, level
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        pvmap, level = ctx.pvmap, ctx.level
        g = g.contiguous()
        g_x = torch.empty((pvmap.n, g.shape[1]), dtype=torch.float32, device=g.device)
        rc = _lib.lib().spv_voxelize_bwd_hip_launcher(pvmap.n, pvmap.n_vox[level], g.shape[1], pvmap.row[level].data_ptr(),
                                                      pvmap.start[level].data_ptr(), g.data_ptr(), g_x.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "spv_voxelize_bwd_hip_launcher")
        return g_x, None, None


# ------------------------------------------------------------------------------------------------------------ public -------
def _check(feat, pvmap, level, rows, what):
    _lib.require_cuda(feat)
    if not isinstance(pvmap, PointVoxelMap):
        raise TypeError("ao_amd spvcnn: %s takes the PointVoxelMap of point_voxel_map(), not %s" % (what, type(pvmap).__name__))
    if not 0 <= level < LEVELS:
        raise ValueError("ao_amd spvcnn: level %r (0..%d)" % (level, LEVELS - 1))
    want = pvmap.n_vox[level] if rows == "voxels" else pvmap.n
    if feat.dim() != 2 or feat.shape[0] != want:
        raise ValueError("ao_amd spvcnn: %s input must be (%d, C), got %s" % (what, want, tuple(feat.shape)))


def devoxelize(feat, pvmap, level, add=None):
    """feat (n_level, C) voxel rows -> (n, C) point rows; add (n, C) is summed into the result (its gradient is the output's)"""
    _check(feat, pvmap, level, "voxels", "devoxelize")
    if add is not None:
        _lib.require_cuda(add)
        if tuple(add.shape) != (pvmap.n, feat.shape[1]):
            raise ValueError("ao_amd spvcnn: devoxelize add must be (%d, %d), got %s" % (pvmap.n, feat.shape[1], tuple(add.shape)))
    if mode() == "torch":
        return devoxelize_torch(feat, pvmap, level, add)
    c = feat.shape[1]
    if c % 32 or not 32 <= c <= MAX_CHANNELS:  # a missing kernel is an error, not a fall-back
        raise ValueError("ao_amd spvcnn: no devoxelize kernel for C = %d (multiples of 32 up to %d)" % (c, MAX_CHANNELS))
    return _Devoxelize.apply(feat, add, pvmap, level)


def voxelize(feat, pvmap, level):
    """feat (n, C) point rows -> (n_level, C): the mean over the points of each voxel"""
    _check(feat, pvmap, level, "points", "voxelize")
    if mode() == "torch":
        return voxelize_torch(feat, pvmap, level)
    c = feat.shape[1]
    if not (1 <= c <= SMALL_CHANNELS or (c % 32 == 0 and 32 <= c <= MAX_CHANNELS)):
        raise ValueError("ao_amd spvcnn: no voxelize kernel for C = %d (1..%d, or multiples of 32 up to %d)"
                         % (c, SMALL_CHANNELS, MAX_CHANNELS))
    return _Voxelize.apply(feat, pvmap, level)
