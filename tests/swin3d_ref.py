"""Swin3D's window attention with cRSE as plain torch, one dense (m, m) problem per window, for any dtype (DESIGN.md section 21
states the function; the extension that defines it is not available).  The table rows always come from the fp32 subtraction of
the signals, so a float64 run and an fp32 run read the same rows."""
import torch


def rows_of(sig, table_rows):
    """(m, m, D) rows of the flat (R, H, hd) tables for the members of one window, sig (m, D)"""
    s = sig.float()
    diff = torch.floor(s[:, None, :] - s[None, :, :])
    out, base = [], 0
    for g, L in enumerate(table_rows):
        for ax in range(3):
            out.append(base + ax * 2 * L + (diff[..., 3 * g + ax] + L).clamp(0, 2 * L - 1).long())
        base += 6 * L
    return torch.stack(out, -1)


def attention(qkv, parts, signals, q_table, k_table, v_table, table_rows, scale, H):
    """qkv (n, 3 C), signals (n, D) and the result (n, C) in the voxels' own order; parts: the rows of each window"""
    n, hd = qkv.shape[0], qkv.shape[1] // (3 * H)
    q, k, v = qkv.view(n, 3, H, hd).unbind(1)
    q = q * scale
    tq, tk, tv = (t.view(-1, H, hd) for t in (q_table, k_table, v_table))
    rows, outs = [], []
    for part in parts:
        idx = torch.as_tensor(part, device=qkv.device)
        r = rows_of(signals[idx], table_rows)
        TQ, TK, TV = (sum(t[r[..., d]] for d in range(r.shape[-1])) for t in (tq, tk, tv))   # (m, m, H, hd)
        e = torch.einsum("ihe,jhe->ijh", q[idx], k[idx]) + (q[idx][:, None] * TQ).sum(-1) + (k[idx][None] * TK).sum(-1)
        p = torch.softmax(e, dim=1)
        outs.append((p[..., None] * (v[idx][None] + TV)).sum(1))
        rows.append(idx)
    return torch.zeros(n, H, hd, dtype=qkv.dtype, device=qkv.device).index_copy(0, torch.cat(rows), torch.cat(outs)).view(n, H * hd)
