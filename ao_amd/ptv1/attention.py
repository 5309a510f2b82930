"""Point Transformer V1's vector attention: everything between the q / k / v Linears and the Bottleneck's bn2.

Reference: pointcept/models/point_transformer/point_transformer_seg.py:45-78.  With C channels, I = C / 8, ns neighbours,
j = idx[n, s] and valid = j >= 0:

    rel  = (coord[j] - coord[n]) * valid                          (n, ns, 3)
    p_r  = linear_p(rel)            Linear(3, 3), BN, ReLU, Linear(3, C)
    r    = x_k[j] * valid - x_q[n] + p_r                          (n, ns, C)
    w    = softmax over ns of linear_w(r)    BN, ReLU, Linear(C, I), BN, ReLU, Linear(I, I)      -1 slots take part
    out[n, s * I + i] = sum over t of (x_v[j] * valid + p_r)[n, t, s * I + i] * w[n, t, i]

The three norms are training-mode BatchNorms over the n * ns rows (the reference's `LayerNorm1d` subclasses BatchNorm1d).

The HIP path is ao_amd/csrc/ptv1.hip (C ABI: include/ptv2_ptv1_hip.h): no (n, ns, C) tensor exists in either direction, the
saved state is two (n, ns, I) tensors.  AO_AMD_PTV1=torch runs the same mathematics in eager torch on the device (the A/B path
of the parity tests, as AO_AMD_PP2S=torch).  There is no CPU fallback on either path.
"""
import ctypes
import os

import torch
import torch.nn.functional as F

from .. import _abi, _lib

_K = _abi.ptv1_consts
SHARE, MAX_NS = _K["PTV1_SHARE"], _K["PTV1_MAX_NS"]
WIDTHS = (32, 64, 128, 256, 512)
_S = _abi.ptv1_structs

# the order of the parameters in ptv1_params / ptv1_grads: (module path, attribute)
PARAMS = (("linear_p.0", "weight"), ("linear_p.0", "bias"), ("linear_p.1", "weight"), ("linear_p.1", "bias"),
          ("linear_p.3", "weight"), ("linear_p.3", "bias"), ("linear_w.0", "weight"), ("linear_w.0", "bias"),
          ("linear_w.2", "weight"), ("linear_w.2", "bias"), ("linear_w.3", "weight"), ("linear_w.3", "bias"),
          ("linear_w.5", "weight"), ("linear_w.5", "bias"))
STAT_KEYS = ("mean3", "var3", "meanc", "varc", "meani", "vari")


def _use_hip():
    return os.environ.get("AO_AMD_PTV1", "hip") != "torch"


def _norms(linear_p, linear_w):
    return linear_p[1], linear_w[0], linear_w[3]


def _params(linear_p, linear_w):
    mods = {"linear_p": linear_p, "linear_w": linear_w}
    out = []
    for path, attr in PARAMS:
        seq, at = path.split(".")
        out.append(getattr(mods[seq][int(at)], attr))
    return out


def _rows_norm(x, bn, stats, key):
    """the reference's LayerNorm1d on (n, ns, c): a BatchNorm over the n * ns rows"""
    rows = x.reshape(-1, x.shape[-1])
    training = bn.training or bn.running_mean is None
    if stats is not None:
        if training:
            stats["mean" + key], stats["var" + key] = rows.mean(0).detach(), rows.var(0, unbiased=False).detach()
        else:
            stats["mean" + key], stats["var" + key] = bn.running_mean.clone(), bn.running_var.clone()
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    y = F.batch_norm(rows, bn.running_mean if (not bn.training or bn.track_running_stats) else None,
                     bn.running_var if (not bn.training or bn.track_running_stats) else None, bn.weight, bn.bias, training,
                     bn.momentum, bn.eps)
    return y.reshape(x.shape)


def attention_torch(x_q, x_k, x_v, coord, idx, linear_p, linear_w, stats=None):
    """The layer in eager torch, operator for operator as the reference (the grouped tensors are (n, ns, C))."""
    n, c = x_q.shape
    i = c // SHARE
    valid = (idx >= 0).unsqueeze(-1).to(x_q.dtype)
    j = idx.clamp(min=0).long()
    rel = (coord[j] - coord.unsqueeze(1)) * valid
    p_r = linear_p[0](rel)
    p_r = linear_p[3](F.relu(_rows_norm(p_r, linear_p[1], stats, "3")))
    r = x_k[j] * valid - x_q.unsqueeze(1) + p_r
    w = linear_w[2](F.relu(_rows_norm(r, linear_w[0], stats, "c")))
    w = linear_w[5](F.relu(_rows_norm(w, linear_w[3], stats, "i")))
    w = torch.softmax(w, dim=1)
    val = (x_v[j] * valid + p_r).reshape(n, -1, SHARE, i)
    return torch.einsum("ntsi,nti->nsi", val, w).reshape(n, c)


class _Sink:
    """carries the caller's `stats` dict through autograd.Function.apply as it is (custom_fwd copies containers)"""

    def __init__(self, stats):
        self.stats = stats


def _struct(name, tensors):
    return _S[name](*[_lib.ptr(t) for t in tensors])


class _VectorAttention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x_q, x_k, x_v, coord, idx, norms, stats, *params):
        from ..ptv2 import gva

        x_q, x_k, x_v, coord = (t.contiguous() for t in (x_q, x_k, x_v, coord))
        params = [p.contiguous() for p in params]
        n, c = x_q.shape
        ns = idx.shape[1]
        i = c // SHARE
        dev = x_q.device
        L = _lib.lib()
        if len({bn.training for bn in norms}) != 1:
            raise ValueError("ao_amd ptv1: the three norms of a layer are in one mode")
        training = norms[0].training
        if training:
            if n * ns < 2:
                raise ValueError("ao_amd ptv1: a training-mode BatchNorm needs more than one row")
            batch = torch.empty(2 * (3 + c + i), dtype=torch.float32, device=dev)
            use = list(batch.split([3, 3, c, c, i, i]))
            track = [bn.track_running_stats and bn.running_mean is not None for bn in norms]
            run = [getattr(bn, a) if t else None for a in ("running_mean", "running_var") for bn, t in zip(norms, track)]
            run = [run[0], run[3], run[1], run[4], run[2], run[5]]  # (mean, var) per norm
            count = [bn.num_batches_tracked if t else None for bn, t in zip(norms, track)]
        else:
            use = [t for bn in norms for t in (bn.running_mean, bn.running_var)]
            run, count = [None] * 6, [None] * 3
        momentum = norms[0].momentum
        if any(bn.momentum != momentum or bn.eps != norms[0].eps for bn in norms) or momentum is None:
            raise ValueError("ao_amd ptv1: the three norms share one eps and one (numeric) momentum")
        p_struct = _struct("ptv1_params", params)
        n_struct = _struct("ptv1_norms", use + run + count)
        saved = torch.empty(max(L.ptv1_attention_saved_bytes(n, ns, c), 256), dtype=torch.uint8, device=dev)
        ws = _lib.workspace(L.ptv1_attention_workspace_bytes(n, ns, c), dev)
        out = torch.empty((n, c), dtype=torch.float32, device=dev)
        rc = L.ptv1_attention_forward_hip_launcher(
            n, ns, c, x_q.data_ptr(), x_k.data_ptr(), x_v.data_ptr(), coord.data_ptr(), idx.data_ptr(),
            ctypes.addressof(p_struct), ctypes.addressof(n_struct), int(training), float(norms[0].eps), float(momentum),
            out.data_ptr(), saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "ptv1_attention_forward_hip_launcher")
        if stats.stats is not None:
            stats.stats.update({k: t.clone() for k, t in zip(STAT_KEYS, use)})
        inv = gva.inverse_table(idx) if any(ctx.needs_input_grad) else ()
        ctx.training, ctx.eps = training, float(norms[0].eps)
        ctx.save_for_backward(x_q, x_k, x_v, coord, idx, saved, *use, *params, *inv)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable  # (raw launches: a second derivative raises instead of being wrong)
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_out):
        x_q, x_k, x_v, coord, idx, saved = ctx.saved_tensors[:6]
        use, params, (inv_ptr, inv_rows) = ctx.saved_tensors[6:12], ctx.saved_tensors[12:26], ctx.saved_tensors[26:]
        n, c = x_q.shape
        ns = idx.shape[1]
        dev = x_q.device
        L = _lib.lib()
        g_out = g_out.contiguous()
        g_x = torch.empty((3, n, c), dtype=torch.float32, device=dev)
        grads = [torch.empty_like(p) for p in params]
        p_struct = _struct("ptv1_params", params)
        n_struct = _struct("ptv1_norms", list(use) + [None] * 9)
        g_struct = _struct("ptv1_grads", grads)
        ws = _lib.workspace(L.ptv1_attention_workspace_bytes(n, ns, c), dev)
        rc = L.ptv1_attention_backward_hip_launcher(
            n, ns, c, x_q.data_ptr(), x_k.data_ptr(), x_v.data_ptr(), coord.data_ptr(), idx.data_ptr(), inv_ptr.data_ptr(),
            inv_rows.data_ptr(), ctypes.addressof(p_struct), ctypes.addressof(n_struct), int(ctx.training), ctx.eps,
            g_out.data_ptr(), saved.data_ptr(), saved.numel(), g_x[0].data_ptr(), g_x[1].data_ptr(), g_x[2].data_ptr(),
            ctypes.addressof(g_struct), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "ptv1_attention_backward_hip_launcher")
        return (g_x[0], g_x[1], g_x[2], None, None, None, None, *grads)


def vector_attention(x_q, x_k, x_v, coord, idx, linear_p, linear_w, stats=None):
    """x_q, x_k, x_v (n, C) -> (n, C).  coord (n, 3) float32; idx (n, ns) int32 with -1 padding (the level's self-kNN table);
    linear_p / linear_w: the layer's two nn.Sequential (their norms' buffers are updated in training mode, as the reference
    does).  stats: a dict that receives the statistics the three norms used (mean3, var3, meanc, varc, meani, vari)."""
    _lib.require_cuda(x_q, x_k, x_v, coord, idx)
    n, c = x_q.shape
    if c not in WIDTHS or idx.dim() != 2 or idx.shape[0] != n or not 1 <= idx.shape[1] <= MAX_NS or idx.dtype != torch.int32:
        raise ValueError("ao_amd ptv1: C must be one of %s and idx (n, ns <= %d) int32; got C = %d, idx %s %s"
                         % (WIDTHS, MAX_NS, c, tuple(idx.shape), idx.dtype))
    if tuple(x_k.shape) != (n, c) or tuple(x_v.shape) != (n, c) or tuple(coord.shape) != (n, 3):
        raise ValueError("ao_amd ptv1: x_q, x_k, x_v must be (n, C) and coord (n, 3)")
    if not _use_hip():
        with torch.autocast("cuda", enabled=False):
            return attention_torch(x_q.float(), x_k.float(), x_v.float(), coord.float(), idx, linear_p, linear_w, stats)
    return _VectorAttention.apply(x_q, x_k, x_v, coord.float(), idx.contiguous(), _norms(linear_p, linear_w), _Sink(stats),
                                  *_params(linear_p, linear_w))
