"""Plain references of OctFormer's dense octree convolutions (ao_amd/csrc/oct_conv.hip) for any dtype, and the tables between two
octree depths built from coordinate dictionaries (numpy), never from the HIP tables."""
import numpy as np
import torch

OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]   # slot (dx + 1) 9 + (dy + 1) 3 + dz + 1


def rows_of(xyz, batch):
    return {(b,) + tuple(p): i for i, (b, p) in enumerate(zip(batch.tolist(), xyz.tolist()))}


def dict_neighbours(xyz, batch):
    rows = rows_of(xyz, batch)
    return np.array([[rows.get((b, x + dx, y + dy, z + dz), -1) for dx, dy, dz in OFFSETS]
                     for b, (x, y, z) in zip(batch.tolist(), xyz.tolist())], np.int32)


def hierarchy(xyz, batch):
    """children in (cloud, key) order -> dict(pxyz, pbatch, parent, child, up, down3): the parents are the distinct coord >> 1 in
    the order of their first child (which is their own (cloud, key) order)"""
    seen = {}
    for b, p in zip(batch.tolist(), (xyz >> 1).tolist()):
        seen.setdefault((b,) + tuple(p), len(seen))
    pbatch = np.array([k[0] for k in seen], np.int64)
    pxyz = np.array([k[1:] for k in seen], np.int64)
    parent = np.array([seen[(b,) + tuple(p)] for b, p in zip(batch.tolist(), (xyz >> 1).tolist())], np.int32)
    child = np.full((len(seen), 8), -1, np.int32)
    child[parent, 4 * (xyz[:, 0] & 1) + 2 * (xyz[:, 1] & 1) + (xyz[:, 2] & 1)] = np.arange(len(xyz))
    kids = rows_of(xyz, batch)
    # up[j, k]: the parent q with 2 q + d == c_j per axis; down3[p, k]: the child at 2 p + d
    up = np.array([[seen.get((b,) + tuple((c - d) // 2), -1) if not ((c - d) & 1).any() else -1 for d in np.array(OFFSETS)]
                   for b, c in zip(batch.tolist(), xyz)], np.int32)
    down3 = np.array([[kids.get((b,) + tuple(2 * p + d), -1) for d in np.array(OFFSETS)] for b, p in zip(pbatch.tolist(), pxyz)], np.int32)
    return dict(pxyz=pxyz, pbatch=pbatch, parent=parent, child=child, up=up, down3=down3)


def conv(x, weights, bias, tab, transpose):
    """out[i] = bias + sum_s x[tab[i, s]] W[s], W[s] = weights[s] (Cin, Cout), or weights[s]^T of a (Cout, Cin) with `transpose`"""
    out = x.new_zeros((tab.shape[0], weights.shape[1] if transpose else weights.shape[2]))
    for s in range(tab.shape[1]):
        j = tab[:, s].long()
        rows = (j >= 0).nonzero().view(-1)
        out = out.index_add(0, rows, x[j[rows]] @ (weights[s].t() if transpose else weights[s]))
    return out if bias is None else out + bias
