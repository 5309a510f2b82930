"""Swin3D's window attention with contextual relative signal encoding (cRSE) on ao_amd/csrc/swin_attention.hip (C ABI
include/ptv2_swin_hip.h), one autograd node.

`crse_attention` is what WindowAttention.forward hands to SelfAttnAIOFunction in the reference (swin3d_layers.py:539-568), an
operator of the external Swin3D package whose source is not available: the function is restated from the paper and the shapes
of swin3d_layers.py and is NOT checked against that extension (DESIGN.md section 21 says what is unpinned).  For i, j of one
window, head h, q already multiplied by scale:

    r_d(i, j) = clamp(floor(signals[i, d] - signals[j, d]) + L_d, 0, 2 L_d - 1)         (one fp32 subtraction; crse_rows)
    T_X(i, j) = sum_d X_table[group(d)][axis(d), r_d(i, j), h, :]
    e_ij = q_i . k_j + q_i . T_Q(i, j) + k_j . T_K(i, j),  p_i. = softmax_j e_ij,  out_i = sum_j p_ij (v_j + T_V(i, j))

The kernels gather qkv through wmap.order and write out in the voxels' original order; no (M, 9) index tensor, no (M, H, hd)
gather and no pair list exists.  The node saves out and the row log-sum-exp (n, H), nothing per pair.

`fp16_mode` (the reference's constructor argument; 0 by default): with 1 or 2 and a float16 `qkv` -- what the qkv Linear writes
under fp16 autocast -- the call runs on ao_amd/csrc/swin_attention_f16.hip (include/ptv2_swin_f16_hip.h):
qkv, out, g_out and g_qkv stay float16 in memory, the tables are rounded to half once as a workgroup stages them, q . k runs on
the fp16 matrix instruction, and everything else is fp32 arithmetic.  That is the reference's mode 1, "fp16 forward and fp32
backward".  Mode 2, "fp16 both ways", takes the SAME path: a half-precision backward is not built.  Every other combination
(fp16_mode 0, a bfloat16, fp32 or float64 qkv) takes the fp32 path: under autocast that node casts its inputs to fp32.

AO_AMD_SWIN3D (read on every call): unset or "hip": the kernels; "torch": the same function as eager statements over explicit
pair lists built from the map, on the device.
"""
import os

import torch

from .. import _abi, _lib
from .window import C as CONSTS, WindowMap, run

MAX_HEADS, MAX_ROWS, MAX_GROUPS = (CONSTS[k] for k in ("SWIN_MAX_HEADS", "SWIN_MAX_ROWS", "SWIN_MAX_GROUPS"))
F16_ARGS = _abi.swin_f16_structs["swin_f16_args"]


def mode():
    m = os.environ.get("AO_AMD_SWIN3D", "hip")
    if m not in ("hip", "torch"):
        raise ValueError("ao_amd swin3d: AO_AMD_SWIN3D=%r (hip or torch)" % m)
    return m


def crse_rows(sig_i, sig_j, table_rows):
    """(M, D) int64 rows of the flat (R, H, hd) tables that the pairs read: python's one statement of the index (the device's
    is swin_row of swin_attention.hip).  sig_i, sig_j (M, D) fp32."""
    L = torch.tensor([l for l in table_rows for _ in range(3)], dtype=torch.float32, device=sig_i.device)
    row0, base = [], 0
    for l in table_rows:
        row0 += [base, base + 2 * l, base + 4 * l]
        base += 6 * l
    r = torch.minimum((torch.floor(sig_i.float() - sig_j.float()) + L).clamp(min=0), 2 * L - 1)
    return r.long() + torch.tensor(row0, device=sig_i.device)


def window_pairs(wmap):
    """(qi, kj) int64: every ordered pair of sorted positions that share a window"""
    m = (wmap.offsets[1:] - wmap.offsets[:-1]).long()
    start = wmap.offsets[:-1].long()
    per = torch.repeat_interleave(m, m)            # (n): the size of each position's window
    first = torch.repeat_interleave(start, m)      # (n): its first position
    qi = torch.repeat_interleave(torch.arange(wmap.n, device=m.device), per)
    pair0 = torch.cumsum(per, 0) - per
    kj = first[qi] + torch.arange(qi.shape[0], device=m.device) - pair0[qi]
    return qi, kj


def crse_attention_torch(qkv, wmap, signals, q_table, k_table, v_table, table_rows, scale, num_heads):
    """the eager statements, for any dtype of qkv and the tables; the rows always come from the fp32 subtraction"""
    n, H = qkv.shape[0], num_heads
    hd = qkv.shape[1] // (3 * H)
    order = wmap.order.long()
    q, k, v = qkv[order].view(n, 3, H, hd).unbind(1)
    q = q * scale
    qi, kj = window_pairs(wmap)
    rows = crse_rows(signals[qi], signals[kj], table_rows)
    tq, tk, tv = (t.reshape(-1, H, hd)[rows].sum(1) for t in (q_table, k_table, v_table))
    e = (q[qi] * k[kj]).sum(-1) + (q[qi] * tq).sum(-1) + (k[kj] * tk).sum(-1)
    top = torch.full((n, H), float("-inf"), dtype=e.dtype, device=e.device).scatter_reduce(0, qi[:, None].expand_as(e), e.detach(), "amax")
    p = torch.exp(e - top[qi])
    p = p / torch.zeros_like(top).index_add(0, qi, p)[qi]
    out = torch.zeros_like(q).index_add(0, qi, p.unsqueeze(-1) * (v[kj] + tv))
    return torch.zeros_like(out).index_copy(0, order, out).view(n, H * hd)


class _Attention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, qkv, q_table, k_table, v_table, signals, wmap, table_rows, scale, num_heads):
        qkv, q_table, k_table, v_table = (t.contiguous() for t in (qkv, q_table, k_table, v_table))
        n, c, h = qkv.shape[0], qkv.shape[1] // 3, num_heads
        out = torch.empty((n, c), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((n, h), dtype=torch.float32, device=qkv.device)
        ctx.fields = dict(n=n, windows=wmap.W, c=c, h=h, hd=c // h, groups=len(table_rows), rows=tuple(table_rows), scale=float(scale),
                          order=wmap.order, offsets=wmap.offsets, signals=signals)
        run("swin_attention_fwd_hip_launcher", "crse_attention", qkv=qkv, q_table=q_table, k_table=k_table, v_table=v_table, out=out,
            lse=lse, **ctx.fields)
        ctx.save_for_backward(qkv, q_table, k_table, v_table, out, lse)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        qkv, q_table, k_table, v_table, out, lse = ctx.saved_tensors
        f = ctx.fields
        g_qkv, g_q, g_k, g_v = (torch.empty_like(t) for t in (qkv, q_table, k_table, v_table))
        need = _lib.lib().ptv2_swin_workspace_bytes(f["n"], f["windows"], f["h"], f["hd"], 6 * sum(f["rows"]))
        ws = _lib.workspace(need, qkv.device)
        run("swin_attention_bwd_hip_launcher", "crse_attention", qkv=qkv, q_table=q_table, k_table=k_table, v_table=v_table, out=out,
            lse=lse, g_out=g.contiguous(), g_qkv=g_qkv, g_q_table=g_q, g_k_table=g_k, g_v_table=g_v, workspace=ws,
            workspace_bytes=ws.numel(), **f)
        return g_qkv, g_q, g_k, g_v, None, None, None, None, None


class _AttentionHalf(torch.autograd.Function):
    """float16 qkv, out, g_out and g_qkv; fp32 tables, table gradients and log-sum-exp (no cast_inputs: half stays half)"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, qkv, q_table, k_table, v_table, signals, wmap, table_rows, scale, num_heads):
        qkv, q_table, k_table, v_table = (t.contiguous() for t in (qkv, q_table, k_table, v_table))
        n, c, h = qkv.shape[0], qkv.shape[1] // 3, num_heads
        out = torch.empty((n, c), dtype=torch.float16, device=qkv.device)
        lse = torch.empty((n, h), dtype=torch.float32, device=qkv.device)
        ctx.fields = dict(n=n, windows=wmap.W, c=c, h=h, hd=c // h, groups=len(table_rows), rows=tuple(table_rows), scale=float(scale),
                          order=wmap.order, offsets=wmap.offsets, signals=signals)
        run("swin_attention_f16_fwd_hip_launcher", "crse_attention", F16_ARGS, qkv=qkv, q_table=q_table, k_table=k_table,
            v_table=v_table, out=out, lse=lse, **ctx.fields)
        ctx.save_for_backward(qkv, q_table, k_table, v_table, out, lse)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        qkv, q_table, k_table, v_table, out, lse = ctx.saved_tensors
        f = ctx.fields
        g_qkv, g_q, g_k, g_v = (torch.empty_like(t) for t in (qkv, q_table, k_table, v_table))
        need = _lib.lib().ptv2_swin_f16_workspace_bytes(f["n"], f["windows"], f["h"], f["hd"], 6 * sum(f["rows"]))
        ws = _lib.workspace(need, qkv.device)
        run("swin_attention_f16_bwd_hip_launcher", "crse_attention", F16_ARGS, qkv=qkv, q_table=q_table, k_table=k_table,
            v_table=v_table, out=out, lse=lse, g_out=g.half().contiguous(), g_qkv=g_qkv, g_q_table=g_q, g_k_table=g_k, g_v_table=g_v,
            workspace=ws, workspace_bytes=ws.numel(), **f)
        return g_qkv, g_q, g_k, g_v, None, None, None, None, None


def crse_attention(qkv, wmap, signals, q_table, k_table, v_table, table_rows, scale, num_heads, fp16_mode=0):
    """(n, C) in the voxels' original order from qkv (n, 3 C), columns [3][H][hd], in original order; `signals` (n, 3 S) fp32 in
    the SORTED order of `wmap`; each table the flat concatenation of its groups' (3, 2 L_s, H, hd) blocks; `table_rows` the
    tuple of L_s.  The flat tables do not tell H from hd, hence `num_heads`.  hd in {8, 16}, H <= 64, sum_s 6 L_s <= 400:
    ValueError otherwise.  `fp16_mode` in {0, 1, 2}: with 1 or 2 a float16 qkv takes the half-precision path and the result is
    float16 (the module docstring states its roundings); anything else takes the fp32 path."""
    _lib.require_cuda(qkv, signals, q_table, k_table, v_table)
    if fp16_mode not in (0, 1, 2):
        raise ValueError("ao_amd swin3d: fp16_mode %r; 0, 1 or 2" % (fp16_mode,))
    if not isinstance(wmap, WindowMap):
        raise TypeError("ao_amd swin3d: crse_attention takes the WindowMap of window_map()")
    rows, H = tuple(int(l) for l in table_rows), int(num_heads)
    if not 1 <= len(rows) <= MAX_GROUPS or min(rows) < 1:
        raise ValueError("ao_amd swin3d: table_rows %r; 1 to %d positive row counts" % (rows, MAX_GROUPS))
    R = 6 * sum(rows)
    if R > MAX_ROWS:
        raise ValueError("ao_amd swin3d: the tables have %d rows per head; at most %d" % (R, MAX_ROWS))
    if not 1 <= H <= MAX_HEADS:
        raise ValueError("ao_amd swin3d: %d heads; at most %d" % (H, MAX_HEADS))
    if qkv.dim() != 2 or qkv.shape[0] != wmap.n or qkv.shape[1] % (3 * H):
        raise ValueError("ao_amd swin3d: qkv is (n, 3 C) with n = %d and C a multiple of %d heads; got %s" % (wmap.n, H, tuple(qkv.shape)))
    C = qkv.shape[1] // 3
    if C // H not in (8, 16):
        raise ValueError("ao_amd swin3d: %d channels per head; 8 or 16" % (C // H))
    if tuple(signals.shape) != (wmap.n, 3 * len(rows)) or signals.dtype != torch.float32:
        raise ValueError("ao_amd swin3d: signals is fp32 (n, %d); got %s %s" % (3 * len(rows), signals.dtype, tuple(signals.shape)))
    for name, t in (("q_table", q_table), ("k_table", k_table), ("v_table", v_table)):
        if t.numel() != R * C:
            raise ValueError("ao_amd swin3d: %s of table_rows %r holds %d x %d x %d values; got %d" % (name, rows, R, H, C // H, t.numel()))
    signals = signals.contiguous()
    if fp16_mode and qkv.dtype == torch.float16:
        with torch.autocast("cuda", enabled=False):
            tables = [t.float() for t in (q_table, k_table, v_table)]
            if mode() == "torch":   # the eager statements in fp32 on the values the kernels read (a table's rounding has
                # the gradient of the identity, as in the kernels); out rounded once
                tables = [t + (t.half().float() - t).detach() for t in tables]
                return crse_attention_torch(qkv.float(), wmap, signals, *tables, rows, scale, H).half()
            return _AttentionHalf.apply(qkv, *tables, signals, wmap, rows, scale, H)
    if mode() == "torch":
        with torch.autocast("cuda", enabled=False):   # fp32 at least; a float64 caller (the tests' reference run) stays float64
            dt = torch.promote_types(qkv.dtype, torch.float32)
            return crse_attention_torch(qkv.to(dt), wmap, signals, q_table.to(dt), k_table.to(dt), v_table.to(dt), rows, scale, H)
    # the fp32 kernels read fp32 memory: outside autocast (where custom_fwd casts nothing) any other dtype is cast here
    return _Attention.apply(*(t.float() for t in (qkv, q_table, k_table, v_table)), signals, wmap, rows, scale, H)
