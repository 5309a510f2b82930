"""The window map of Swin3D's window attention on ao_amd/csrc/swin_map.hip.

`window_map` restates BasicLayer.get_map_pair, get_window_mapping and get_shifted_sp (swin3d_layers.py:714-843 of the reference)
without MinkowskiEngine: the window of a voxel is floor_div(grid_coord + shift, window_size) per axis with the cloud as a fourth
axis, its slot (grid_coord + shift) mod window_size.  One kernel forms the 64-bit (cloud, window, slot) key, torch.sort orders
the keys, a second kernel marks the first voxel of every window, a scan numbers the windows and a third kernel writes the CSR.
The order of the windows themselves is that of their keys (the reference's comes from a hash map and is free).
"""
import ctypes

import torch

from .. import _abi, _lib

C = _abi.swin_consts
ARGS = _abi.swin_structs["swin_args"]
MAX_WINDOW = C["SWIN_MAX_WINDOW"]


def run(launcher, what, struct=ARGS, **fields):
    a = struct()
    for name, value in fields.items():
        if name == "rows":
            for s, v in enumerate(value):
                a.rows[s] = v
        else:
            setattr(a, name, value.data_ptr() if torch.is_tensor(value) else value)
    rc = getattr(_lib.lib(), launcher)(ctypes.addressof(a), _lib.stream_ptr())
    _lib.check(rc, "%s for %s" % (launcher, what))


class WindowMap:
    """`order` (n) int32: the voxels sorted by window, then by w_w_id ascending (the reference's n2n_indices); `offsets` (W + 1)
    int32: a CSR over the windows in sorted positions; `w_w_xyz` (n, 3) int32 in sorted order; `W` windows, the largest of
    `m_max` members; `window_size`, `shift`."""

    def __init__(self, order, offsets, w_w_xyz, W, m_max, window_size, shift):
        self.order, self.offsets, self.w_w_xyz = order, offsets, w_w_xyz
        self.W, self.m_max, self.window_size, self.shift = W, m_max, window_size, shift

    @property
    def n(self):
        return self.order.shape[0]


@torch.no_grad()
def window_map(grid_coord, batch, window_size, shift=0):
    """grid_coord (n, 3) integer voxel coordinates at the level's own stride 1, batch (n) integer, both on the device.  Two
    voxels of one cloud on one coordinate, a cloud id outside [0, 32768) or a window coordinate outside [-4096, 4096) raise
    ValueError (one read-back)."""
    _lib.require_cuda(grid_coord, batch)
    if grid_coord.dim() != 2 or grid_coord.shape[1] != 3 or batch.shape != grid_coord.shape[:1] or grid_coord.shape[0] < 1:
        raise ValueError("ao_amd swin3d: window_map takes grid_coord (n, 3) and batch (n), n >= 1; got %s %s"
                         % (tuple(grid_coord.shape), tuple(batch.shape)))
    if grid_coord.is_floating_point() or batch.is_floating_point():
        raise ValueError("ao_amd swin3d: window_map takes integer coordinates and cloud ids")
    ws, shift = int(window_size), int(shift)
    if not 1 <= ws <= MAX_WINDOW:
        raise ValueError("ao_amd swin3d: window_size %d outside [1, %d]" % (ws, MAX_WINDOW))
    if not 0 <= shift < ws:
        raise ValueError("ao_amd swin3d: shift %d outside [0, window_size)" % shift)
    n, dev = grid_coord.shape[0], grid_coord.device
    g, b = grid_coord.int().contiguous(), batch.int().contiguous()
    if (g != grid_coord).any() or (b != batch).any():
        raise ValueError("ao_amd swin3d: a coordinate or a cloud id does not fit 32 bits")
    stat = torch.zeros(4, dtype=torch.int32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    run("swin_map_keys_hip_launcher", "window_map", n=n, window_size=ws, shift=shift, grid_coord=g, batch=b, keys_out=keys, stat=stat)
    keys, order = torch.sort(keys)
    head = torch.empty(n, dtype=torch.int32, device=dev)
    w_w_xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
    run("swin_map_heads_hip_launcher", "window_map", n=n, window_size=ws, keys=keys, head_out=head, w_w_xyz_out=w_w_xyz, stat=stat)
    wid = torch.cumsum(head, 0, dtype=torch.int32)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    run("swin_map_offsets_hip_launcher", "window_map", n=n, window_size=ws, head=head, wid=wid, offsets_out=offsets, stat=stat)
    bad, dup, W, m_max = stat.tolist()
    if bad:
        raise ValueError("ao_amd swin3d: a cloud id lies outside [0, %d) or a window coordinate outside [-%d, %d)"
                         % (C["SWIN_MAX_CLOUDS"], C["SWIN_WINDOW_BIAS"], C["SWIN_WINDOW_BIAS"]))
    if dup:
        raise ValueError("ao_amd swin3d: two voxels of one cloud share a coordinate")
    return WindowMap(order.int().contiguous(), offsets[:W + 1].clone(), w_w_xyz, W, m_max, ws, shift)
