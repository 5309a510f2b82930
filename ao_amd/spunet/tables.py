"""The neighbour tables of a voxelised batch: one library call per forward (ao_amd/csrc/spconv_tables.hip, C ABI
include/ptv2_spconv_hip.h) builds the stem's k = 5 table, the k = 3 table of each of the five levels and, per downsampling,
child / parent / slot, the coarse coordinates and the coarse offset.  One host read-back: the five counts and the status words.

`SpconvTables` objects come from `build_tables` only: the convolutions of ao_amd/spunet/conv.py take such an object and a key,
never a table tensor of the caller's.
"""
import ctypes

import torch

from .. import _abi, _lib

_K = _abi.spconv_consts
LEVELS = _K["SPCONV_LEVELS"]
COORD_BITS = _K["SPCONV_COORD_BITS"]
MAX_CLOUDS = _K["SPCONV_MAX_CLOUDS"]
_WORDS = _K["SPCONV_STATUS_WORDS"]
_MESSAGES = ("a negative coordinate", "a coordinate of 2^%d or more" % COORD_BITS, "two rows of one cloud on the same voxel")
_TOKEN = object()

# table builds since import (tests/test_gpu_spunet_model.py: one per forward)
BUILDS = 0


class SpconvTables:
    """n[l], coord[l] (n_l, 3), offset[l] (b), nbr3[l] (n_l, 27) for the five levels; nbr5 (n_0, 125); child[l] (n_{l+1}, 8),
    parent[l] (n_l) and slot[l] (n_l) for the four downsamplings.  int32, on the device, read-only."""

    def __init__(self, token, **fields):
        if token is not _TOKEN:
            raise TypeError("ao_amd spunet: SpconvTables are made by build_tables()")
        self.__dict__.update(fields)

    def lookup(self, indice_key, level, kernel_size):
        """(kind, level) of an spconv `indice_key` at `level`: "stem" is the k = 5 table of level 0, "subm<l>" the k = 3 table
        of level l, "spconv<l>" the downsampling from level l - 1 to l; None: by level and kernel size"""
        if indice_key is None:
            return ("subm5", 0) if kernel_size == 5 else ("subm3", level)
        if indice_key == "stem":
            return ("subm5", 0)
        for prefix, kind, shift in (("subm", "subm3", 0), ("spconv", "down", 1)):
            if indice_key.startswith(prefix) and indice_key[len(prefix):].isdigit():
                at = int(indice_key[len(prefix):]) - shift
                if 0 <= at < LEVELS - shift:
                    return kind, at
        raise KeyError("ao_amd spunet: no table for indice_key %r" % (indice_key,))


def build_tables(discrete_coord, offset):
    """discrete_coord (n, 3) integer voxel coordinates in [0, 2^18), unique within a cloud; offset (b) cloud ends."""
    global BUILDS
    _lib.require_cuda(discrete_coord, offset)
    if discrete_coord.dim() != 2 or discrete_coord.shape[1] != 3 or discrete_coord.is_floating_point():
        raise ValueError("ao_amd spunet: discrete_coord must be (n, 3) integers, got %s %s"
                         % (tuple(discrete_coord.shape), discrete_coord.dtype))
    n, b = discrete_coord.shape[0], offset.numel()
    if n < 1 or not 1 <= b <= MAX_CLOUDS or offset.dim() != 1:
        raise ValueError("ao_amd spunet: %d voxels in %d clouds (at least one voxel, 1..%d clouds)" % (n, b, MAX_CLOUDS))
    dev = discrete_coord.device
    if discrete_coord.dtype != torch.int32:
        # (int64 coordinates beyond int32 would wrap: clamp them to a value the library reports as too large)
        discrete_coord = discrete_coord.clamp(-1, 1 << COORD_BITS).int()
    coord0 = discrete_coord.contiguous()
    offset0 = offset.int().contiguous()
    L = _lib.lib()
    per_row = 125 + 27 * LEVELS + (8 + 1 + 1 + 3) * (LEVELS - 1)
    store = torch.empty(n * per_row + b * (LEVELS - 1), dtype=torch.int32, device=dev)
    meta = torch.zeros(LEVELS + _WORDS, dtype=torch.int32, device=dev)
    at = 0

    def take(count):
        nonlocal at
        out = store[at:at + count]
        at += count
        return out

    nbr5 = take(n * 125)
    nbr3 = [take(n * 27) for _ in range(LEVELS)]
    child = [take(n * 8) for _ in range(LEVELS - 1)]
    parent = [take(n) for _ in range(LEVELS - 1)]
    slot = [take(n) for _ in range(LEVELS - 1)]
    coord = [take(n * 3) for _ in range(LEVELS - 1)]
    offs = [take(b) for _ in range(LEVELS - 1)]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    struct = _abi.spconv_structs["spconv_tables"](nbr5.data_ptr(), ptrs(nbr3), ptrs(child), ptrs(parent), ptrs(slot), ptrs(coord),
                                                  ptrs(offs), meta.data_ptr(), meta[LEVELS:].data_ptr())
    ws = _lib.workspace(L.ptv2_spconv_tables_workspace_bytes(n, b), dev)
    rc = L.spconv_build_tables_hip_launcher(n, b, coord0.data_ptr(), offset0.data_ptr(), ctypes.addressof(struct), ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "spconv_build_tables_hip_launcher")
    BUILDS += 1
    host = meta.tolist()  # THE read-back of the forward: five counts, three status words
    bad = [m for m, word in zip(_MESSAGES, host[LEVELS:]) if word]
    if bad:
        raise ValueError("ao_amd spunet: discrete_coord has " + ", ".join(bad))
    counts = host[:LEVELS]
    return SpconvTables(
        _TOKEN, n=counts, clouds=b, coord=[coord0] + [coord[l][:3 * counts[l + 1]].view(-1, 3) for l in range(LEVELS - 1)],
        offset=[offset0] + offs, nbr5=nbr5.view(n, 125), nbr3=[nbr3[l][:27 * counts[l]].view(-1, 27) for l in range(LEVELS)],
        child=[child[l][:8 * counts[l + 1]].view(-1, 8) for l in range(LEVELS - 1)],
        parent=[parent[l][:counts[l]] for l in range(LEVELS - 1)], slot=[slot[l][:counts[l]] for l in range(LEVELS - 1)])
