"""Node order and per-depth tables of OctFormer's blocks.

`octree_level` sorts the non-empty nodes of one depth by (cloud, Morton key), the order in which OctFormer cuts them into
patches, and builds the 27-neighbour table of the depthwise convolution on ao_amd/csrc/oct_dwconv.hip.

`xyz2key` is ocnn's key convention restated from its documentation (ocnn is not available to check it against): bit i of x goes
to key bit 3 i + 2, y to 3 i + 1, z to 3 i.  It is the only place python forms a key; oct_key of oct_dwconv.hip is the device's
copy, and the neighbour table is wrong wherever the two differ.
"""
import ctypes

import torch

from .. import _abi, _lib

C = _abi.oct_consts
ARGS = _abi.oct_structs["oct_args"]
MAX_DEPTH = C["OCT_MAX_DEPTH"]


def run(launcher, what, **fields):
    a = ARGS()
    for name, value in fields.items():
        setattr(a, name, value.data_ptr() if torch.is_tensor(value) else value)
    rc = getattr(_lib.lib(), launcher)(ctypes.addressof(a), _lib.stream_ptr())
    _lib.check(rc, "%s for %s" % (launcher, what))


def xyz2key(x, y, z, depth):
    """int64 Morton key of integer coordinates in [0, 2^depth)"""
    x, y, z = x.long(), y.long(), z.long()
    key = torch.zeros_like(x)
    for i in range(depth):
        key = key | ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return key


class OctreeLevel:
    """The nodes of one depth in (cloud, Morton key) order: `order` (n) int64, the permutation that sorts the caller's rows;
    `xyz` (n, 3) int32, `batch` (n) int32 and `keys` (n) int64 in that order; `cloud_offsets` (clouds + 1) int32; `nbr` (n, 27)
    int32; `clouds`, `depth`."""

    def __init__(self, order, xyz, batch, keys, cloud_offsets, nbr, clouds, depth):
        self.order, self.xyz, self.batch, self.keys = order, xyz, batch, keys
        self.cloud_offsets, self.nbr, self.clouds, self.depth = cloud_offsets, nbr, clouds, depth

    @property
    def n(self):
        return self.xyz.shape[0]


@torch.no_grad()
def octree_level(grid_coord, batch, depth):
    """grid_coord (n, 3) integer, batch (n) integer, both on the device.  Coordinates must lie in [0, 2^depth) and be unique
    within a cloud: ValueError otherwise (one read-back)."""
    _lib.require_cuda(grid_coord, batch)
    if grid_coord.dim() != 2 or grid_coord.shape[1] != 3 or batch.shape != grid_coord.shape[:1] or grid_coord.shape[0] < 1:
        raise ValueError("ao_amd octformer: octree_level takes grid_coord (n, 3) and batch (n), n >= 1; got %s %s"
                         % (tuple(grid_coord.shape), tuple(batch.shape)))
    if grid_coord.is_floating_point() or batch.is_floating_point():
        raise ValueError("ao_amd octformer: octree_level takes integer coordinates and cloud ids")
    depth = int(depth)
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError("ao_amd octformer: depth %d outside [1, %d]" % (depth, MAX_DEPTH))
    n, dev = grid_coord.shape[0], grid_coord.device
    g, b = grid_coord.long(), batch.long()
    key = xyz2key(g[:, 0], g[:, 1], g[:, 2], depth)
    full, order = torch.sort(b << (3 * depth) | key)
    in_range = ((g >= 0) & (g < 2 ** depth)).all() & (b >= 0).all()
    unique = (full[1:] != full[:-1]).all()
    in_range, unique, clouds = (int(v) for v in torch.stack([in_range.long(), unique.long(), b.max() + 1]).tolist())
    if not in_range:
        raise ValueError("ao_amd octformer: a coordinate lies outside [0, 2^%d) or a cloud id is negative" % depth)
    if not unique:
        raise ValueError("ao_amd octformer: two nodes of one cloud share a coordinate")
    xyz, bat = g[order].int().contiguous(), b[order].int().contiguous()
    keys = (full & ((1 << (3 * depth)) - 1)).contiguous()
    counts = torch.bincount(bat.long(), minlength=clouds)
    cloud_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int().contiguous()
    nbr = torch.empty((n, 27), dtype=torch.int32, device=dev)
    run("oct_neighbors_hip_launcher", "octree_level", n=n, clouds=clouds, depth=depth, xyz=xyz, batch=bat, keys=keys,
        cloud_offsets=cloud_offsets, nbr_out=nbr)
    return OctreeLevel(order, xyz, bat, keys, cloud_offsets, nbr, clouds, depth)


# ------------------------------------------------------------------------------------ the hierarchy ----
TABLES = _abi.octconv_structs["octconv_tables"]


class OctreeLink:
    """The tables between the children (depth d, n rows) and the parents (depth d - 1, n_parent rows) of include/
    ptv2_octconv_hip.h, all int32: `parent` (n), `child` (n_parent, 8), `onehot` (n, 8), `up` (n, 27), `down3` (n_parent, 27)."""

    def __init__(self, parent, child, onehot, up, down3):
        self.parent, self.child, self.onehot, self.up, self.down3 = parent, child, onehot, up, down3

    @property
    def n(self):
        return self.parent.shape[0]

    @property
    def n_parent(self):
        return self.child.shape[0]


class OctreePyramid:
    """`levels[i]` is the OctreeLevel of depth `depth - i`; `links[i]` the OctreeLink between levels[i] (children) and
    levels[i + 1] (parents)."""

    def __init__(self, levels, links, depth):
        self.levels, self.links, self.depth = levels, links, depth

    def level(self, depth):
        if not self.depth - len(self.levels) < depth <= self.depth:
            raise ValueError("ao_amd octformer: depth %d is not in this pyramid (%d .. %d)" % (depth, self.depth - len(self.levels) + 1, self.depth))
        return self.levels[self.depth - depth]

    def link(self, depth):
        """between the children at `depth` and their parents at depth - 1"""
        if not self.depth - len(self.levels) + 1 < depth <= self.depth:
            raise ValueError("ao_amd octformer: no link below depth %d in this pyramid (%d .. %d)" % (depth, self.depth - len(self.levels) + 1, self.depth))
        return self.links[self.depth - depth]


@torch.no_grad()
def octree_link(child, parent):
    """The OctreeLink of two neighbouring OctreeLevels, `parent` being octree_level() of the unique coord >> 1 of `child`: in
    (cloud, key) order the children of a node are consecutive, so one thread per parent walks them (no search); up and down3
    go through `parent.nbr`.  Three small kernels of oct_conv.hip."""
    n, m, dev = child.n, parent.n, child.xyz.device
    pk = (child.batch.long() << (3 * child.depth) | child.keys) >> 3
    first = torch.cat([pk.new_ones(1), (pk[1:] != pk[:-1]).long()]).nonzero().view(-1)
    if first.numel() != m:
        raise ValueError("ao_amd octformer: %d nodes at depth %d have %d parents, the level above has %d" % (n, child.depth, first.numel(), m))
    first = torch.cat([first, first.new_full((1,), n)]).int().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    link = OctreeLink(torch.empty(n, **i32), torch.empty((m, 8), **i32), torch.empty((n, 8), **i32), torch.empty((n, 27), **i32),
                      torch.empty((m, 27), **i32))
    a = TABLES()
    a.n, a.n_parent = n, m
    for name, t in (("keys", child.keys), ("xyz", child.xyz), ("first", first), ("parent_nbr", parent.nbr), ("parent", link.parent),
                    ("child", link.child), ("onehot", link.onehot), ("up", link.up), ("down3", link.down3)):
        setattr(a, name, t.data_ptr())
    rc = _lib.lib().oct_conv_tables_hip_launcher(ctypes.addressof(a), _lib.stream_ptr())
    _lib.check(rc, "oct_conv_tables_hip_launcher for octree_link")
    return link


@torch.no_grad()
def octree_pyramid(grid_coord, batch, depth, levels):
    """The OctreeLevel of every depth `depth`, depth - 1, .., depth - levels + 1 and the OctreeLink between neighbours.  Each
    coarser level is octree_level() of the unique coord >> 1 of the level above (the first child of every run of equal parent
    keys gives the coordinate)."""
    depth, levels = int(depth), int(levels)
    if not 1 <= levels <= depth:
        raise ValueError("ao_amd octformer: %d levels from depth %d; between 1 and the depth" % (levels, depth))
    out, links = [octree_level(grid_coord, batch, depth)], []
    for _ in range(levels - 1):
        child = out[-1]
        pk = (child.batch.long() << (3 * child.depth) | child.keys) >> 3
        head = torch.cat([pk.new_ones(1), (pk[1:] != pk[:-1]).long()]).nonzero().view(-1)
        out.append(octree_level(child.xyz[head] >> 1, child.batch[head], child.depth - 1))
        links.append(octree_link(child, out[-1]))
    return OctreePyramid(out, links, depth)
