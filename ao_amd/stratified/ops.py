"""Stratified Transformer's operators on ao_amd/csrc/stratified.hip (C ABI include/ptv2_st_hip.h).

`build_pairs` makes the (query, key) lists of stratified window attention on the device without a (windows, k, k) mask,
`window_attention` is the whole of WindowAttention.forward between the qkv projection and the output projection as one autograd
node, and `attention_step1_v2`, `dot_prod_with_idx_v3`, `attention_step2_with_rel_pos_value_v2` are the three pointops2 operators
the reference model calls, with `scatter_softmax_csr` between them.

AO_AMD_ST (read on every call): unset or "fused": the fused node (16 channels per head; 32 take the staged operators);
"staged": the three operators and the row softmax; "torch": the reference's eager statements on the device.

The pairs of a query are a CSR row: index_0_offsets (N + 1) and index_1 (M), both int32.  The backwards gather by key through
the transposed lists (`transpose_csr`), so the gradients of q, k and v are sums in a fixed order and bit-repeatable; the three
table gradients are summed through float atomics and are not.
"""
import ctypes
import os

import numpy as np
import torch

from .. import _abi, _lib

C = _abi.st_consts
ARGS = _abi.st_structs["st_args"]
MAX_HEADS = C["ST_MAX_HEADS"]
MAX_TABLE_ROWS = C["ST_MAX_TABLE_ROWS"]
_LDS_BYTES = 64 * 1024   # what one workgroup of a table-gradient kernel may take (stratified.hip: ST_MAX_LDS)
_ROWS = 16          # rows one workgroup holds at a time (stratified.hip: ST_ROWS)


def mode():
    m = os.environ.get("AO_AMD_ST", "fused")
    if m not in ("fused", "staged", "torch"):
        raise ValueError("ao_amd stratified: AO_AMD_ST=%r (fused, staged or torch)" % m)
    return m


def _run(op, what, **fields):
    a = ARGS()
    for name, value in fields.items():
        setattr(a, name, value.data_ptr() if torch.is_tensor(value) else value)
    rc = _lib.lib().st_op_hip_launcher(C[op], ctypes.addressof(a), _lib.stream_ptr())
    _lib.check(rc, "st_op_hip_launcher(%s) for %s" % (op, what))


def _check_rows(rows, hd, tables, what):
    need = 4 * (tables * rows * 3 * (hd + 1) + _ROWS * tables * rows * 3)
    if rows < 1 or rows > MAX_TABLE_ROWS or need > _LDS_BYTES:
        raise ValueError("ao_amd stratified: %s with a table of %d rows and %d channels per head needs %d bytes of LDS per "
                         "workgroup (at most %d, and at most %d rows)" % (what, rows, hd, need, _LDS_BYTES, MAX_TABLE_ROWS))


def _check_qkv(what, *ts):
    n, h, hd = ts[0].shape
    for t in ts:
        if t.dim() != 3 or t.shape != (n, h, hd) or t.dtype != torch.float32:
            raise ValueError("ao_amd stratified: %s takes fp32 (N, h, hdim) of one shape (queries and keys are the same points); "
                             "got %s" % (what, [(tuple(x.shape), x.dtype) for x in ts]))
    if hd not in (16, 32) or not 1 <= h <= MAX_HEADS:
        raise ValueError("ao_amd stratified: %s supports hdim 16 and 32 and up to %d heads; got h=%d hdim=%d" % (what, MAX_HEADS, h, hd))
    return n, h, hd


def _tr(table):
    """(L, h, hdim, 3) -> the library's (L, h, 3, hdim)"""
    return table.permute(0, 1, 3, 2).contiguous()


# ------------------------------------------------------------------------------------------------------ pair lists ----
def index_0_of(offsets, m=None):
    """the query of every pair, (M) int64, from the CSR offsets"""
    counts = (offsets[1:] - offsets[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.numel(), device=offsets.device), counts, output_size=m)


def transpose_csr(offsets, index_1, check=True):
    """The pairs by key: (t_offsets (N + 1) int32, t_query (M) int32, t_pair (M) int32).  Slot s of key j is pair t_pair[s] with
    query t_query[s]; the slots of one key ascend by pair, so a sum over them has one order."""
    n, m = offsets.numel() - 1, index_1.numel()
    if check and m and (int(index_1.min()) < 0 or int(index_1.max()) >= n):
        raise ValueError("ao_amd stratified: index_1 names a point outside [0, %d)" % n)
    key = index_1.long()
    t_pair = torch.sort(key, stable=True)[1]
    counts = torch.bincount(key, minlength=n)
    t_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
    t_query = index_0_of(offsets, m)[t_pair].int()
    return t_offsets, t_query.contiguous(), t_pair.int().contiguous()


class PairSet:
    """The pairs of one (level, shift): by query (index_0_offsets, index_1, n_max) and by key (t_offsets, t_query, t_pair)."""

    def __init__(self, index_0_offsets, index_1, n_max, t_offsets, t_query, t_pair):
        self.index_0_offsets, self.index_1, self.n_max = index_0_offsets, index_1, n_max
        self.t_offsets, self.t_query, self.t_pair = t_offsets, t_query, t_pair
        self._index_0 = None

    @property
    def n(self):
        return self.index_0_offsets.numel() - 1

    @property
    def m(self):
        return self.index_1.numel()

    @property
    def index_0(self):
        if self._index_0 is None:
            self._index_0 = index_0_of(self.index_0_offsets, self.m)
        return self._index_0

    @property
    def by_key(self):
        return self.t_offsets, self.t_query, self.t_pair

    @classmethod
    def from_csr(cls, index_0_offsets, index_1):
        """a foreign CSR: the transposition is made here, once"""
        off, idx = index_0_offsets.int().contiguous(), index_1.int().contiguous()
        counts = off[1:] - off[:-1]
        return cls(off, idx, int(counts.max()) if counts.numel() else 0, *transpose_csr(off, idx))


def offset2batch(offset, n):
    return torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)


def cells(coords, start, size, shifted, want_cell=True, want_wcoord=True):
    """(cell, wcoord), each (N, 3) int32 or None: the grid cell trunc(((p + shift) - start) / size) of every point and the
    window coordinate of stratified_transformer_v1m2_refine.py:394-406, in fp32 as the eager statements round.  `size` is
    a python float that is exactly an fp32 value; shift = size / 2 when shifted."""
    _lib.require_cuda(coords, start)
    coords, start = coords.float().contiguous(), start.float().contiguous()
    n = coords.shape[0]
    cell = torch.empty((n, 3), dtype=torch.int32, device=coords.device) if want_cell else None
    wcoord = torch.empty((n, 3), dtype=torch.int32, device=coords.device) if want_wcoord else None
    rc = _lib.lib().st_cells_hip_launcher(n, coords.data_ptr(), start.data_ptr(), float(size), 1 if shifted else 0,
                                          _lib.ptr(cell), _lib.ptr(wcoord), _lib.stream_ptr())
    _lib.check(rc, "st_cells_hip_launcher")
    return cell, wcoord


def _cell_key(cell, batch):
    """one int64 per point that is equal exactly where cell and cloud are (only the partition matters)"""
    c = cell.long()
    c = c - c.amin(0, keepdim=True)
    ext = c.amax(0) + 1
    return ((batch * ext[0] + c[:, 0]) * ext[1] + c[:, 1]) * ext[2] + c[:, 2]


def _segments(key, members):
    """`members` (ascending point indices) sorted by key, ascending within a key -> (order, unique keys, begin, end)"""
    ks, o = torch.sort(key[members], stable=True)
    uniq, cnt = torch.unique_consecutive(ks, return_counts=True)
    end = cnt.cumsum(0)
    return members[o], uniq, end - cnt, end


@torch.no_grad()
def build_pairs(coords, offset, down_idx, window_size, shifted):
    """The pairs of stratified attention (:374-417) as a PairSet.  Keys of query i: every point of i's small window (size
    `window_size`), ascending; then every point of `down_idx` in i's large window (size 2 * window_size) whose window coordinate
    (:394-406) differs from i's in any axis, ascending.  The small and the large grid need not nest.  count -> scan -> fill over
    the points sorted by cell; nothing of size (windows, k) exists.  Two read-backs: M and n_max."""
    _lib.require_cuda(coords, offset, down_idx)
    if coords.dim() != 2 or coords.shape[1] != 3 or offset.dim() != 1 or offset.numel() < 1:
        raise ValueError("ao_amd stratified: build_pairs takes coords (N, 3) and offset (b); got %s %s" % (tuple(coords.shape), tuple(offset.shape)))
    coords = coords.float().contiguous()
    n, dev = coords.shape[0], coords.device
    if n == 0:
        raise ValueError("ao_amd stratified: build_pairs of no point")
    w = np.float32(window_size)
    batch = offset2batch(offset, n)
    start = coords.min(0).values
    cell_s, wcoord = cells(coords, start, float(w), shifted)
    cell_l, _ = cells(coords, start, float(w * np.float32(2)), shifted, want_wcoord=False)
    key_s, key_l = _cell_key(cell_s, batch), _cell_key(cell_l, batch)
    everyone = torch.arange(n, device=dev)
    order_s, uniq_s, beg_s, end_s = _segments(key_s, everyone)
    at = torch.searchsorted(uniq_s, key_s)
    seg_s = torch.stack([beg_s[at], end_s[at]], 1).int().contiguous()
    sampled = torch.unique(down_idx.long())   # ascending, as a mask would read them
    if sampled.numel() and (int(sampled[0]) < 0 or int(sampled[-1]) >= n):
        raise ValueError("ao_amd stratified: down_idx names a point outside [0, %d)" % n)
    nd = sampled.numel()
    if nd:
        order_l, uniq_l, beg_l, end_l = _segments(key_l, sampled)
        at = torch.searchsorted(uniq_l, key_l).clamp(max=uniq_l.numel() - 1)
        hit = uniq_l[at] == key_l
        seg_l = torch.stack([torch.where(hit, beg_l[at], 0), torch.where(hit, end_l[at], 0)], 1).int().contiguous()
    else:
        order_l, seg_l = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((n, 2), dtype=torch.int32, device=dev)
    order_s, order_l = order_s.int().contiguous(), order_l.int().contiguous()
    L = _lib.lib()
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    rc = L.st_pairs_hip_launcher(n, nd, 0, order_s.data_ptr(), seg_s.data_ptr(), order_l.data_ptr(), seg_l.data_ptr(),
                                 wcoord.data_ptr(), counts.data_ptr(), 0, 0, 0, _lib.stream_ptr())
    _lib.check(rc, "st_pairs_hip_launcher (count)")
    ends = counts.long().cumsum(0)
    m, n_max = int(ends[-1]), int(counts.max())
    if m >= 2 ** 31:
        raise ValueError("ao_amd stratified: %d pairs do not fit int32 indices" % m)
    offsets = torch.cat([ends.new_zeros(1), ends]).int().contiguous()
    index_1 = torch.empty(m, dtype=torch.int32, device=dev)
    rc = L.st_pairs_hip_launcher(n, nd, 1, order_s.data_ptr(), seg_s.data_ptr(), order_l.data_ptr(), seg_l.data_ptr(),
                                 wcoord.data_ptr(), 0, offsets.data_ptr(), m, index_1.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "st_pairs_hip_launcher (fill)")
    return PairSet(offsets, index_1, n_max, *transpose_csr(offsets, index_1, check=False))


def quant_grid_length(window_size, quant_size):
    return int((2 * window_size + 1e-4) // quant_size)


def _rel_scalars(window_size, quant_size):
    """2 * window_size and 1 / quant_size as the device's eager statements see them: python scalars rounded to fp32, and a
    division by a python scalar done as a multiplication by the scalar's fp32 reciprocal"""
    return float(np.float32(2 * window_size)), float(np.float32(1.0) / np.float32(quant_size))


@torch.no_grad()
def rel_index(coords, index_0, index_1, window_size, quant_size, rows=None):
    """relative_position_index (M, 3) int32 of :145-151, clamped to [0, rows) (rows defaults to 2 * quant_grid_length)"""
    _lib.require_cuda(coords, index_0, index_1)
    coords = coords.float().contiguous()
    i0, i1 = index_0.int().contiguous(), index_1.int().contiguous()
    rows = 2 * quant_grid_length(window_size, quant_size) if rows is None else int(rows)
    two_w, inv_q = _rel_scalars(window_size, quant_size)
    rel = torch.empty((i0.numel(), 3), dtype=torch.int32, device=coords.device)
    rc = _lib.lib().st_rel_index_hip_launcher(coords.shape[0], i0.numel(), rows, coords.data_ptr(), i0.data_ptr(), i1.data_ptr(),
                                              two_w, inv_q, rel.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "st_rel_index_hip_launcher")
    return rel


def rel_index_torch(coords, index_0, index_1, window_size, quant_size):
    """:145-151, statement for statement (float (M, 3))"""
    relative_position = coords[index_0.long()] - coords[index_1.long()]
    relative_position = torch.round(relative_position * 100000) / 100000
    return torch.div(relative_position + 2 * window_size - 1e-4, quant_size, rounding_mode="trunc")


# --------------------------------------------------------------------------------------- the three pointops2 operators ----
def _csr(offsets, index_1, n, what):
    if offsets.dtype != torch.int32 or index_1.dtype != torch.int32 or offsets.numel() != n + 1:
        raise ValueError("ao_amd stratified: %s takes int32 index0_offsets (N + 1) and index1 (M); got %s %s %s %s for N = %d" % (
            what, tuple(offsets.shape), offsets.dtype, tuple(index_1.shape), index_1.dtype, n))
    return offsets.contiguous(), index_1.contiguous()


class _Step1(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, q, k, index1, index0_offsets, by_key):
        q, k = q.contiguous(), k.contiguous()
        n, h, hd = _check_qkv("attention_step1_v2", q, k)
        off, idx = _csr(index0_offsets, index1, n, "attention_step1_v2")
        m = idx.numel()
        out = torch.empty((m, h), dtype=torch.float32, device=q.device)
        _run("ST_OP_STEP1_FWD", "attention_step1_v2", n=n, h=h, hd=hd, rows=1, m=m, offsets=off, index1=idx, q=q, k=k, attn_out=out)
        ctx.save_for_backward(q, k, off, idx)
        ctx.by_key = by_key
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        q, k, off, idx = ctx.saved_tensors
        (n, h, hd), m = q.shape, idx.numel()
        g = g.contiguous()
        t_off, t_query, t_pair = ctx.by_key if ctx.by_key is not None else transpose_csr(off, idx)
        gq, gk = torch.empty_like(q), torch.empty_like(k)
        _run("ST_OP_STEP1_BWD_Q", "attention_step1_v2", n=n, h=h, hd=hd, rows=1, m=m, offsets=off, index1=idx, k=k, g_attn=g, gq=gq)
        _run("ST_OP_STEP1_BWD_K", "attention_step1_v2", n=n, h=h, hd=hd, rows=1, m=m, t_offsets=t_off, t_query=t_query,
             t_pair=t_pair, q=q, g_attn=g, gk=gk)
        return gq, gk, None, None, None


class _DotProd(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, q, index_q_offsets, k, index_k, table_q, table_k, rel_idx, by_key):
        q, k = q.contiguous(), k.contiguous()
        n, h, hd = _check_qkv("dot_prod_with_idx_v3", q, k)
        off, idx = _csr(index_q_offsets, index_k, n, "dot_prod_with_idx_v3")
        m, rows = idx.numel(), table_q.shape[0]
        if table_q.shape != (rows, h, hd, 3) or table_k.shape != table_q.shape or rel_idx.shape != (m, 3) or rel_idx.dtype != torch.int32:
            raise ValueError("ao_amd stratified: dot_prod_with_idx_v3 takes tables (L, h, hdim, 3) and int32 rel_idx (M, 3); got %s %s %s %s"
                             % (tuple(table_q.shape), tuple(table_k.shape), tuple(rel_idx.shape), rel_idx.dtype))
        _check_rows(rows, hd, 1, "dot_prod_with_idx_v3")
        tq, tk, rel = _tr(table_q), _tr(table_k), rel_idx.contiguous()
        out = torch.empty((m, h), dtype=torch.float32, device=q.device)
        _run("ST_OP_DOT_FWD", "dot_prod_with_idx_v3", n=n, h=h, hd=hd, rows=rows, m=m, offsets=off, index1=idx, rel=rel, q=q, k=k,
             tq=tq, tk=tk, attn_out=out)
        ctx.save_for_backward(q, k, off, idx, tq, tk, rel)
        ctx.by_key = by_key
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        q, k, off, idx, tq, tk, rel = ctx.saved_tensors
        (n, h, hd), m, rows = q.shape, idx.numel(), tq.shape[0]
        g = g.contiguous()
        t_off, t_query, t_pair = ctx.by_key if ctx.by_key is not None else transpose_csr(off, idx)
        gq, gk = torch.empty_like(q), torch.empty_like(k)
        gtq, gtk = torch.zeros_like(tq), torch.zeros_like(tk)
        _run("ST_OP_DOT_BWD_Q", "dot_prod_with_idx_v3", n=n, h=h, hd=hd, rows=rows, m=m, offsets=off, index1=idx, rel=rel, q=q,
             tq=tq, g_attn=g, gq=gq, gtq=gtq)
        _run("ST_OP_DOT_BWD_K", "dot_prod_with_idx_v3", n=n, h=h, hd=hd, rows=rows, m=m, t_offsets=t_off, t_query=t_query,
             t_pair=t_pair, rel=rel, k=k, tk=tk, g_attn=g, gk=gk, gtk=gtk)
        return gq, None, gk, None, _tr(gtq), _tr(gtk), None, None


class _Step2(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, attn, v, index0_offsets, index1, table, rel_idx, by_key):
        attn, v = attn.contiguous(), v.contiguous()
        n, h, hd = _check_qkv("attention_step2_with_rel_pos_value_v2", v)
        off, idx = _csr(index0_offsets, index1, n, "attention_step2_with_rel_pos_value_v2")
        m, rows = idx.numel(), table.shape[0]
        if table.shape != (rows, h, hd, 3) or rel_idx.shape != (m, 3) or rel_idx.dtype != torch.int32 or attn.shape != (m, h) \
                or attn.dtype != torch.float32:
            raise ValueError("ao_amd stratified: attention_step2_with_rel_pos_value_v2 takes fp32 attn (M, h), a table (L, h, hdim, 3) and "
                             "int32 rel_idx (M, 3); got %s %s %s %s" % (tuple(attn.shape), tuple(table.shape), tuple(rel_idx.shape), rel_idx.dtype))
        _check_rows(rows, hd, 1, "attention_step2_with_rel_pos_value_v2")
        tv, rel = _tr(table), rel_idx.contiguous()
        out = torch.empty((n, h, hd), dtype=torch.float32, device=v.device)
        _run("ST_OP_STEP2_FWD", "attention_step2_with_rel_pos_value_v2", n=n, h=h, hd=hd, rows=rows, m=m, offsets=off, index1=idx,
             rel=rel, attn=attn, v=v, tv=tv, out=out)
        ctx.save_for_backward(attn, v, off, idx, tv, rel)
        ctx.by_key = by_key
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        attn, v, off, idx, tv, rel = ctx.saved_tensors
        (n, h, hd), m, rows = v.shape, idx.numel(), tv.shape[0]
        g = g.contiguous()
        t_off, t_query, t_pair = ctx.by_key if ctx.by_key is not None else transpose_csr(off, idx)
        g_attn, gv, gtv = torch.empty_like(attn), torch.empty_like(v), torch.zeros_like(tv)
        _run("ST_OP_STEP2_BWD_Q", "attention_step2_with_rel_pos_value_v2", n=n, h=h, hd=hd, rows=rows, m=m, offsets=off, index1=idx,
             rel=rel, attn=attn, v=v, tv=tv, g_out=g, attn_out=g_attn, gtv=gtv)
        _run("ST_OP_STEP2_BWD_K", "attention_step2_with_rel_pos_value_v2", n=n, h=h, hd=hd, rows=rows, m=m, t_offsets=t_off,
             t_query=t_query, t_pair=t_pair, attn=attn, g_out=g, gv=gv)
        return g_attn, gv, None, None, _tr(gtv), None, None


class _ScatterSoftmax(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, src, index0_offsets):
        src, off = src.contiguous(), index0_offsets.contiguous()
        (m, h), n = src.shape, off.numel() - 1
        out = torch.empty_like(src)
        _run("ST_OP_SOFTMAX_FWD", "scatter_softmax_csr", n=n, h=h, hd=16, rows=1, m=m, offsets=off, attn=src, attn_out=out)
        ctx.save_for_backward(out, off)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        y, off = ctx.saved_tensors
        (m, h), n = y.shape, off.numel() - 1
        g = g.contiguous()
        gx = torch.empty_like(y)
        _run("ST_OP_SOFTMAX_BWD", "scatter_softmax_csr", n=n, h=h, hd=16, rows=1, m=m, offsets=off, attn=y, g_attn=g, attn_out=gx)
        return gx, None


def attention_step1_v2(q, k, index1, index0_offsets, n_max=None, by_key=None):
    """(M, h): q_i . k_j per pair and head (libs/pointops2/functions/pointops.py:169-257).  n_max is accepted and unused: no row
    length is capped.  by_key: the transposed lists of the pairs when the caller has them (PairSet.by_key)."""
    _lib.require_cuda(q, k, index1, index0_offsets)
    return _Step1.apply(q, k, index1, index0_offsets, by_key)


def dot_prod_with_idx_v3(q, index_q_offsets, n_max, k, index_k, table_q, table_k, rel_idx, by_key=None):
    """(M, h): q_i . sum_a table_q[rel[m, a], :, :, a] + k_j . sum_a table_k[rel[m, a], :, :, a] (:631-754)"""
    _lib.require_cuda(q, k, index_k, index_q_offsets, table_q, table_k, rel_idx)
    return _DotProd.apply(q, index_q_offsets, k, index_k, table_q, table_k, rel_idx, by_key)


def attention_step2_with_rel_pos_value_v2(attn, v, index0_offsets, n_max, index1, table, rel_idx, by_key=None):
    """(N, h, hdim): sum over the pairs of a query of attn[m] (v_j + sum_a table[rel[m, a], :, :, a]) (:853-960)"""
    _lib.require_cuda(attn, v, index0_offsets, index1, table, rel_idx)
    return _Step2.apply(attn, v, index0_offsets, index1, table, rel_idx, by_key)


def scatter_softmax_csr(src, index0_offsets):
    """softmax of src (M, h) over the pairs of each query: torch_scatter.scatter_softmax(src, index_0, dim=0) for sorted pairs"""
    _lib.require_cuda(src, index0_offsets)
    if src.dim() != 2 or index0_offsets.dtype != torch.int32:
        raise ValueError("ao_amd stratified: scatter_softmax_csr takes (M, h) and int32 offsets; got %s %s" % (tuple(src.shape), index0_offsets.dtype))
    return _ScatterSoftmax.apply(src, index0_offsets)


# ------------------------------------------------------------------------------------------------ window attention ----
class _WindowAttention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, q, k, v, coords, off, idx, t_off, t_query, table_q, table_k, table_v, window_size, quant_size):
        q, k, v, coords = q.contiguous(), k.contiguous(), v.contiguous(), coords.contiguous()
        n, h, hd = q.shape
        rows, m = table_q.shape[0], idx.numel()
        tq, tk, tv = _tr(table_q), _tr(table_k), _tr(table_v)
        two_w, inv_q = _rel_scalars(window_size, quant_size)
        out = torch.empty((n, h, hd), dtype=torch.float32, device=q.device)
        lse = torch.empty((n, h), dtype=torch.float32, device=q.device)
        _run("ST_OP_FUSED_FWD", "window_attention", n=n, h=h, hd=hd, rows=rows, m=m, two_w=two_w, inv_q=inv_q, offsets=off,
             index1=idx, coords=coords, q=q, k=k, v=v, tq=tq, tk=tk, tv=tv, out=out, lse_out=lse)
        ctx.save_for_backward(q, k, v, coords, off, idx, t_off, t_query, tq, tk, tv, out, lse)
        ctx.scalars = (two_w, inv_q)
        return out.view(n, h * hd)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        q, k, v, coords, off, idx, t_off, t_query, tq, tk, tv, out, lse = ctx.saved_tensors
        (n, h, hd), rows, m = q.shape, tq.shape[0], idx.numel()
        two_w, inv_q = ctx.scalars
        g = g.contiguous().view(n, h, hd)
        delta = (g * out).sum(-1).contiguous()
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        gtq, gtk, gtv = torch.zeros_like(tq), torch.zeros_like(tk), torch.zeros_like(tv)
        common = dict(n=n, h=h, hd=hd, rows=rows, m=m, two_w=two_w, inv_q=inv_q, coords=coords, q=q, k=k, v=v, tq=tq, tk=tk, tv=tv,
                      g_out=g, lse=lse, delta=delta)
        _run("ST_OP_FUSED_BWD_Q", "window_attention", offsets=off, index1=idx, gq=gq, gtq=gtq, gtv=gtv, **common)
        _run("ST_OP_FUSED_BWD_K", "window_attention", t_offsets=t_off, t_query=t_query, gk=gk, gv=gv, gtk=gtk, **common)
        return gq, gk, gv, None, None, None, None, None, _tr(gtq), _tr(gtk), _tr(gtv), None, None


def window_attention_torch(q, k, v, coords, index_0, index_1, table_q, table_k, table_v, window_size, quant_size):
    """WindowAttention.forward :140-202 in eager statements (the pointops2 calls written out as gathers), for any dtype"""
    n, h, hd = q.shape
    i0, i1 = index_0.long(), index_1.long()
    rel = rel_index_torch(coords.float(), i0, i1, window_size, quant_size).long().clamp(0, table_q.shape[0] - 1)

    def lookup(table):  # (M, h, hdim): the sum over the three axes
        return table[rel[:, 0], :, :, 0] + table[rel[:, 1], :, :, 1] + table[rel[:, 2], :, :, 2]

    qi, kj = q[i0], k[i1]
    attn = (qi * kj).sum(-1) + (qi * lookup(table_q)).sum(-1) + (kj * lookup(table_k)).sum(-1)
    with torch.no_grad():  # (the shift of a softmax carries no gradient)
        top = torch.full((n, h), float("-inf"), dtype=attn.dtype, device=attn.device)
        top = top.scatter_reduce(0, i0.view(-1, 1).expand(-1, h), attn, "amax")
    e = torch.exp(attn - top[i0])
    p = e / torch.zeros((n, h), dtype=attn.dtype, device=attn.device).index_add_(0, i0, e)[i0]
    x = torch.zeros((n, h, hd), dtype=attn.dtype, device=attn.device).index_add_(0, i0, p.unsqueeze(-1) * (v[i1] + lookup(table_v)))
    return x.view(n, h * hd)


def window_attention(q, k, v, coords, pairs, table_q, table_k, table_v, window_size, quant_size):
    """(N, h * hdim) of WindowAttention.forward :140-202: per (query, head) the softmax over the query's pairs of
    q . k + q . tq[rel] + k . tk[rel], aggregating v + tv[rel], with rel the relative-position index recomputed from `coords`.
    q is already scaled.  q, k, v (N, h, hdim); pairs a PairSet; tables (L, h, hdim, 3).  fp32, under autocast too.

    The fused node (hdim 16) allocates nothing of M elements: it keeps out and the row log-sum-exp (N, h) for the backward."""
    _lib.require_cuda(q, k, v, coords, table_q, table_k, table_v)
    if not isinstance(pairs, PairSet):
        raise TypeError("ao_amd stratified: window_attention takes a PairSet (build_pairs, or PairSet.from_csr for a foreign CSR)")
    how = mode()
    if how == "torch":
        with torch.autocast("cuda", enabled=False):
            return window_attention_torch(q.float(), k.float(), v.float(), coords, pairs.index_0, pairs.index_1, table_q.float(),
                                          table_k.float(), table_v.float(), window_size, quant_size)
    q, k, v = q.float(), k.float(), v.float()
    n, h, hd = _check_qkv("window_attention", q, k, v)
    rows = table_q.shape[0]
    if pairs.n != n or coords.shape != (n, 3) or any(t.shape != (rows, h, hd, 3) for t in (table_q, table_k, table_v)):
        raise ValueError("ao_amd stratified: window_attention of %d points, %d heads of %d: pairs of %d points, coords %s, tables %s" % (
            n, h, hd, pairs.n, tuple(coords.shape), [tuple(t.shape) for t in (table_q, table_k, table_v)]))
    coords = coords.float()
    if how == "fused" and hd == 16:
        _check_rows(rows, hd, 2, "window_attention")
        return _WindowAttention.apply(q, k, v, coords, pairs.index_0_offsets, pairs.index_1, pairs.t_offsets, pairs.t_query,
                                      table_q, table_k, table_v, float(window_size), float(quant_size))
    with torch.autocast("cuda", enabled=False):
        off, idx, by_key = pairs.index_0_offsets, pairs.index_1, pairs.by_key
        rel = rel_index(coords, pairs.index_0, idx, window_size, quant_size, rows)
        tq, tk, tv = table_q.float(), table_k.float(), table_v.float()
        attn = attention_step1_v2(q, k, idx, off, pairs.n_max, by_key) + dot_prod_with_idx_v3(q, off, pairs.n_max, k, idx, tq, tk, rel, by_key)
        p = scatter_softmax_csr(attn, off)
        return attention_step2_with_rel_pos_value_v2(p, v, off, pairs.n_max, idx, tv, rel, by_key).view(n, h * hd)
