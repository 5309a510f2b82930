"""The point-voxel map of SPVCNN: which voxel of each of the five levels a point lies in, and the points of every voxel.

One library call (ao_amd/csrc/spv_map.hip, C ABI include/ptv2_spv_hip.h) sorts the points once per level by the key of the sparse
convolutions' tables, so a voxel's rank among the distinct keys is its row in `SpconvTables` at every level; one host read-back
(the five voxel counts and the status words) sizes the `build_tables` call on the unique level-0 voxels, which has its own.

`PointVoxelMap` objects come from `point_voxel_map` only.
"""
import ctypes

import torch

from .. import _abi, _lib
from ..spunet.tables import build_tables

_K = _abi.spv_consts
LEVELS = _K["SPV_LEVELS"]
COORD_BITS = _K["SPV_COORD_BITS"]
MAX_CLOUDS = _K["SPV_MAX_CLOUDS"]
_WORDS = _K["SPV_STATUS_WORDS"]
_MESSAGES = ("a negative coordinate", "a coordinate of 2^%d or more" % COORD_BITS)
_TOKEN = object()

# map builds since import (tests/test_gpu_spvcnn_model.py: one per forward)
BUILDS = 0


class PointVoxelMap:
    """n points, clouds; coord (n, 3) and offset (b) as given (int32); tables: the SpconvTables of the unique level-0 voxels
    (tables.coord[0], tables.offset[0]); per level l: row[l] (n) the voxel of each point, start[l] (n_l + 1) and order[l] (n)
    the points of each voxel in ascending index.  int32, on the device, read-only."""

    def __init__(self, token, **fields):
        if token is not _TOKEN:
            raise TypeError("ao_amd spvcnn: PointVoxelMaps are made by point_voxel_map()")
        self.__dict__.update(fields)

    def counts(self, level):
        """(n_level) points per voxel"""
        return self.start[level][1:] - self.start[level][:-1]


def point_voxel_map(discrete_coord, offset):
    """discrete_coord (n, 3) integer point coordinates in [0, 2^18), any number of points per voxel; offset (b) cloud ends."""
    global BUILDS
    _lib.require_cuda(discrete_coord, offset)
    if discrete_coord.dim() != 2 or discrete_coord.shape[1] != 3 or discrete_coord.is_floating_point():
        raise ValueError("ao_amd spvcnn: discrete_coord must be (n, 3) integers, got %s %s"
                         % (tuple(discrete_coord.shape), discrete_coord.dtype))
    n, b = discrete_coord.shape[0], offset.numel()
    if n < 1 or not 1 <= b <= MAX_CLOUDS or offset.dim() != 1:
        raise ValueError("ao_amd spvcnn: %d points in %d clouds (at least one point, 1..%d clouds)" % (n, b, MAX_CLOUDS))
    dev = discrete_coord.device
    if discrete_coord.dtype != torch.int32:
        discrete_coord = discrete_coord.clamp(-1, 1 << COORD_BITS).int()
    coord = discrete_coord.contiguous()
    offset = offset.int().contiguous()
    L = _lib.lib()
    store = torch.empty(LEVELS * (3 * n + 1) + 3 * n + b, dtype=torch.int32, device=dev)
    meta = torch.zeros(LEVELS + _WORDS, dtype=torch.int32, device=dev)
    at = 0

    def take(count):
        nonlocal at
        out = store[at:at + count]
        at += count
        return out

    row = [take(n) for _ in range(LEVELS)]
    start = [take(n + 1) for _ in range(LEVELS)]
    order = [take(n) for _ in range(LEVELS)]
    vcoord, voffset = take(3 * n), take(b)
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    struct = _abi.spv_structs["spv_map"](ptrs(row), ptrs(start), ptrs(order), vcoord.data_ptr(), voffset.data_ptr(),
                                         meta.data_ptr(), meta[LEVELS:].data_ptr())
    ws = _lib.workspace(L.ptv2_spv_map_workspace_bytes(n, b), dev)
    rc = L.spv_build_map_hip_launcher(n, b, coord.data_ptr(), offset.data_ptr(), ctypes.addressof(struct), ws.data_ptr(), ws.numel(),
                                      _lib.stream_ptr())
    _lib.check(rc, "spv_build_map_hip_launcher")
    BUILDS += 1
    host = meta.tolist()  # THE read-back of the map: five counts, two status words
    bad = [m for m, word in zip(_MESSAGES, host[LEVELS:]) if word]
    if bad:
        raise ValueError("ao_amd spvcnn: discrete_coord has " + ", ".join(bad))
    counts = host[:LEVELS]
    tables = build_tables(vcoord[:3 * counts[0]].view(-1, 3), voffset)
    if tables.n != counts:  # (both are on the host already)
        raise RuntimeError("ao_amd spvcnn: the map has %s voxels per level, the tables %s" % (counts, tables.n))
    return PointVoxelMap(_TOKEN, n=n, clouds=b, coord=coord, offset=offset, tables=tables, n_vox=counts, row=row,
                         start=[start[l][:counts[l] + 1] for l in range(LEVELS)], order=order)
