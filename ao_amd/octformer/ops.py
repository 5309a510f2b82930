"""OctFormer's two hot operators on ao_amd/csrc/oct_attention.hip and oct_dwconv.hip (C ABI include/ptv2_oct_hip.h; DESIGN.md
section 19), each one autograd node.

`octree_attention` is OctreeAttention.forward between the qkv projection and the output projection: the dilated patch partition,
the logits with the three-axis relative-position bias, the per-cloud mask, the row softmax, the aggregation and the reverse
partition, without a padded or transposed copy of the nodes, a mask, an index tensor or a (P, H, K, K) tensor.  It saves out and
the row log-sum-exp (n, H).  `octree_dwconv` is the depthwise convolution over the 27-neighbour table.

AO_AMD_OCTFORMER (read on every call): unset or "hip": the kernels; "torch": the reference's eager statements on the device.
"""
import ctypes
import os

import torch

from .. import _abi, _lib
from .octree import C as CONSTS, OctreeLevel, OctreeLink, run

MAX_PATCH, MAX_HEADS, MAX_RPE, MAX_CHANNELS = (CONSTS[k] for k in ("OCT_MAX_PATCH", "OCT_MAX_HEADS", "OCT_MAX_RPE", "OCT_MAX_CHANNELS"))


def mode():
    m = os.environ.get("AO_AMD_OCTFORMER", "hip")
    if m not in ("hip", "torch"):
        raise ValueError("ao_amd octformer: AO_AMD_OCTFORMER=%r (hip or torch)" % m)
    return m


def _wide(t):
    """the eager path's operand: fp32, or float64 as it is (the float64 run of a whole model)"""
    return t if t.dtype == torch.float64 else t.float()


def pos_bnd_of(patch_size, dilation):
    return int(0.8 * patch_size * dilation ** 0.5)


# ------------------------------------------------------------------------------------------------------- attention ----
class _Attention(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, qkv, table, level, patch, dilation, scale):
        qkv, table = qkv.contiguous(), table.contiguous()
        n, h = qkv.shape[0], table.shape[1]
        c = qkv.shape[1] // 3
        out = torch.empty((n, c), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((n, h), dtype=torch.float32, device=qkv.device)
        ctx.shape = dict(n=n, c=c, h=h, hd=c // h, patch=patch, dilation=dilation, pos_bnd=pos_bnd_of(patch, dilation),
                         scale=float(scale))
        ctx.level = level
        run("oct_attention_fwd_hip_launcher", "octree_attention", xyz=level.xyz, batch=level.batch, qkv=qkv, table=table, out=out,
            lse=lse, **ctx.shape)
        ctx.save_for_backward(qkv, table, out, lse)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        qkv, table, out, lse = ctx.saved_tensors
        s, level = ctx.shape, ctx.level
        g = g.contiguous()
        g_qkv, g_table = torch.empty_like(qkv), torch.empty_like(table)
        need = _lib.lib().ptv2_oct_workspace_bytes(s["n"], s["patch"], s["dilation"], s["h"], 2 * s["pos_bnd"] + 1)
        ws = _lib.workspace(need, qkv.device)
        run("oct_attention_bwd_hip_launcher", "octree_attention", xyz=level.xyz, batch=level.batch, qkv=qkv, table=table, out=out,
            lse=lse, g_out=g, g_qkv=g_qkv, g_table=g_table, workspace=ws, workspace_bytes=ws.numel(), **s)
        return g_qkv, g_table, None, None, None, None


def octree_attention_torch(qkv, xyz, batch, clouds, table, patch_size, dilation, scale):
    """OctreeT.build_t and OctreeAttention.forward (octformer_v1m1_base.py:56-99, :165-176, :212-245) in eager statements on a
    qkv that is already projected, for any dtype.  The padded rows are zeros where the reference's carry the qkv bias: they
    attend only each other and patch_reverse cuts them off."""
    K, D, H = patch_size, dilation, table.shape[1]
    n, C = qkv.shape[0], qkv.shape[1] // 3
    num = -(-n // (K * D)) * (K * D) - n
    pos_bnd = pos_bnd_of(K, D)
    rpe_num = 2 * pos_bnd + 1

    def patch_partition(data, fill_value=0):
        return torch.cat([data, data.new_full((num,) + data.shape[1:], fill_value)], dim=0)

    batch, xyz, data = patch_partition(batch.long(), clouds), patch_partition(xyz.long()), patch_partition(qkv)
    if D > 1:
        mask = batch.view(-1, K, D).transpose(1, 2).reshape(-1, K)
        xyz = xyz.view(-1, K, D, 3).transpose(1, 2).reshape(-1, K, 3)
        data = data.view(-1, K, D, 3 * C).transpose(1, 2).reshape(-1, 3 * C)
    else:
        mask, xyz = batch.view(-1, K), xyz.view(-1, K, 3)
    mask = mask.unsqueeze(2) - mask.unsqueeze(1)
    mask = mask.masked_fill(mask != 0, -1e3)
    rel_pos = xyz.unsqueeze(2) - xyz.unsqueeze(1)

    q, k, v = data.reshape(-1, K, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q = q * scale
    attn = q @ k.transpose(-2, -1)
    idx = rel_pos.clamp(-pos_bnd, pos_bnd) + (pos_bnd + torch.arange(3, device=xyz.device) * rpe_num)
    rpe = table.index_select(0, idx.reshape(-1)).view(idx.shape + (-1,)).sum(3).permute(0, 3, 1, 2)
    attn = torch.softmax(attn + rpe + mask.unsqueeze(1), dim=-1)
    data = (attn @ v).transpose(1, 2).reshape(-1, C)
    if D > 1:
        data = data.view(-1, D, K, C).transpose(1, 2).reshape(-1, C)
    return data[:n]


def octree_attention(qkv, level, table, patch_size, dilation, scale):
    """(n, C) from qkv (n, 3 C) in the order of `level`, columns [3][H][hd], and the table (3 R, H), R = 2 pos_bnd + 1,
    pos_bnd = int(0.8 K sqrt(D)).  fp32, under autocast too."""
    _lib.require_cuda(qkv, table)
    if not isinstance(level, OctreeLevel):
        raise TypeError("ao_amd octformer: octree_attention takes the OctreeLevel of octree_level()")
    K, D = int(patch_size), int(dilation)
    if not 1 <= K <= MAX_PATCH:
        raise ValueError("ao_amd octformer: patch_size %d outside [1, %d]" % (K, MAX_PATCH))
    if D < 1:
        raise ValueError("ao_amd octformer: dilation %d; at least 1" % D)
    R = 2 * pos_bnd_of(K, D) + 1
    if R > MAX_RPE:
        raise ValueError("ao_amd octformer: patch_size %d with dilation %d has %d table rows per axis; at most %d" % (K, D, R, MAX_RPE))
    if table.dim() != 2 or table.shape[0] != 3 * R:
        raise ValueError("ao_amd octformer: the table of patch_size %d, dilation %d is (%d, H); got %s" % (K, D, 3 * R, tuple(table.shape)))
    H = table.shape[1]
    if not 1 <= H <= MAX_HEADS:
        raise ValueError("ao_amd octformer: %d heads; at most %d" % (H, MAX_HEADS))
    if qkv.dim() != 2 or qkv.shape[0] != level.n or qkv.shape[1] % (3 * H):
        raise ValueError("ao_amd octformer: qkv is (n, 3 C) with n = %d and C a multiple of %d heads; got %s" % (level.n, H, tuple(qkv.shape)))
    hd = qkv.shape[1] // (3 * H)
    if hd not in (16, 32):
        raise ValueError("ao_amd octformer: %d channels per head; 16 or 32" % hd)
    if mode() == "torch":
        with torch.autocast("cuda", enabled=False):
            return octree_attention_torch(_wide(qkv), level.xyz, level.batch, level.clouds, _wide(table), K, D, scale)
    return _Attention.apply(qkv, table, level, K, D, scale)


# ----------------------------------------------------------------------------------------------------- convolution ----
class _DWConv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weights, level):
        x, w = x.contiguous(), weights.contiguous()
        y = torch.empty_like(x)
        run("oct_dwconv_fwd_hip_launcher", "octree_dwconv", n=x.shape[0], c=x.shape[1], nbr=level.nbr, x=x, w=w, y=y)
        ctx.save_for_backward(x, w)
        ctx.level = level
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        (n, c), g = x.shape, g.contiguous()
        g_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        ws = _lib.workspace(_lib.lib().ptv2_oct_dwconv_workspace_bytes(n, c), x.device)
        run("oct_dwconv_bwd_hip_launcher", "octree_dwconv", n=n, c=c, nbr=ctx.level.nbr, x=x, w=w, g_y=g, g_x=_lib.ptr(g_x),
            g_w=_lib.ptr(g_w), workspace=ws, workspace_bytes=ws.numel())
        return g_x, g_w, None


def octree_dwconv_torch(x, weights, nbr):
    """the 27 slots one after the other, for any dtype"""
    y = torch.zeros_like(x)
    for k in range(27):
        j = nbr[:, k].long()
        y = y + weights[k, 0] * torch.where((j >= 0).unsqueeze(1), x[j.clamp(min=0)], torch.zeros_like(x))
    return y


def octree_dwconv(x, weights, level):
    """(n, C): y[i, c] = sum_k weights[k, 0, c] x[nbr[i, k], c] over the 27 neighbours of `level`, missing ones skipped."""
    _lib.require_cuda(x, weights)
    if not isinstance(level, OctreeLevel):
        raise TypeError("ao_amd octformer: octree_dwconv takes the OctreeLevel of octree_level()")
    if x.dim() != 2 or x.shape[0] != level.n or tuple(weights.shape) != (27, 1, x.shape[1]):
        raise ValueError("ao_amd octformer: octree_dwconv takes x (n, C) with n = %d and weights (27, 1, C); got %s %s"
                         % (level.n, tuple(x.shape), tuple(weights.shape)))
    if x.shape[1] % 4 or not 4 <= x.shape[1] <= MAX_CHANNELS:
        raise ValueError("ao_amd octformer: %d channels; a multiple of 4, at most %d" % (x.shape[1], MAX_CHANNELS))
    if mode() == "torch":
        with torch.autocast("cuda", enabled=False):
            return octree_dwconv_torch(_wide(x), _wide(weights), level.nbr)
    return _DWConv.apply(x, weights, level)


# ----------------------------------------------------------------------- dense convolutions ----
CONV_ARGS = _abi.octconv_structs["octconv_args"]
CONV_BF16_ARGS = _abi.octconv_bf16_structs["octconv_bf16_args"]   # the same fields (include/ptv2_octconv_bf16_hip.h)
CONV_MAX, CONV_STEM = (_abi.octconv_consts[k] for k in ("OCTCONV_MAX_CHANNELS", "OCTCONV_STEM_CHANNELS"))
FORMS = ("conv3", "down2", "deconv3")
OPERANDS = ("fp32", "bf16", "autocast")


def conv_tables(table, form):
    """(forward table, weights read transposed, input-gradient table, its transpose flag, its reverse flag) of a form: `table`
    is the OctreeLevel of a "conv3" (k = 3, stride 1) and the OctreeLink of a "down2" (k = 2, stride 2: children to parents)
    or a "deconv3" (k = 3, stride 2 deconvolution: parents to children)."""
    if form not in FORMS:
        raise ValueError("ao_amd octformer: form %r; one of %s" % (form, ", ".join(FORMS)))
    if not isinstance(table, OctreeLevel if form == "conv3" else OctreeLink):
        raise TypeError("ao_amd octformer: a %s takes the %s" % (form, "OctreeLevel of its depth" if form == "conv3" else "OctreeLink above / below its depth"))
    if form == "conv3":
        return table.nbr, 0, table.nbr, 1, 1
    if form == "down2":
        return table.child, 0, table.onehot, 1, 0
    return table.up, 1, table.down3, 0, 0


def run_conv(launcher, bf16=False, **fields):
    """`launcher` is "fwd", "gx" or "gw": of oct_conv.hip, or with bf16 operands of oct_conv_bf16.hip"""
    launcher = "oct_conv_%s%s_hip_launcher" % ("bf16_" if bf16 else "", launcher)
    a = (CONV_BF16_ARGS if bf16 else CONV_ARGS)()
    for name, value in fields.items():
        setattr(a, name, value.data_ptr() if torch.is_tensor(value) else value)
    rc = getattr(_lib.lib(), launcher)(ctypes.addressof(a), _lib.stream_ptr())
    _lib.check(rc, "%s for octree_conv" % launcher)


class _Conv(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weights, bias, table, form, cin, cout, bf16):
        x, w = x.contiguous(), weights.contiguous()
        b = None if bias is None else bias.contiguous()
        tab, transpose = conv_tables(table, form)[:2]
        out = torch.empty((tab.shape[0], cout), dtype=torch.float32, device=x.device)
        run_conv("fwd", bf16, n_out=tab.shape[0], n_in=x.shape[0], slots=tab.shape[1], cin=cin, cout=cout,
                 transpose=transpose, tab=tab, x=x, w=w, bias=_lib.ptr(b), out=out)
        ctx.save_for_backward(x, w)
        ctx.args = (table, form, cin, cout, b is not None, bf16)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        table, form, cin, cout, has_bias, bf16 = ctx.args
        tab, transpose, gtab, gtranspose, reverse = conv_tables(table, form)
        g = g.contiguous()
        g_x = g_w = g_b = None
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(x)
            run_conv("gx", bf16, n_out=x.shape[0], n_in=g.shape[0], slots=gtab.shape[1], cin=cin, cout=cout,
                     transpose=gtranspose, reverse=reverse, tab=gtab, x=g, w=w, out=g_x)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            g_w = torch.empty_like(w)
            g_b = torch.empty(cout, dtype=torch.float32, device=x.device) if has_bias else None
            L = _lib.lib()
            need = (L.ptv2_octconv_bf16_workspace_bytes if bf16 else L.ptv2_octconv_workspace_bytes)(g.shape[0], tab.shape[1], cin, cout)
            ws = _lib.workspace(need, x.device)
            run_conv("gw", bf16, n_out=g.shape[0], n_in=x.shape[0], slots=tab.shape[1], cin=cin, cout=cout,
                     transpose=transpose, tab=tab, x=x, g=g, g_w=g_w, g_b=_lib.ptr(g_b), workspace=ws, workspace_bytes=ws.numel())
        return g_x, g_w, g_b, None, None, None, None, None


def octree_conv_torch(x, weights, bias, tab, transpose):
    """out[i] = bias + sum_s x[tab[i, s]] W[s] (W[s] transposed with `transpose`), the slots one after the other, for any dtype"""
    out = x.new_zeros((tab.shape[0], weights.shape[1] if transpose else weights.shape[2]))
    for s in range(tab.shape[1]):
        j = tab[:, s].long()
        rows = (j >= 0).nonzero().view(-1)
        out = out.index_add(0, rows, x[j[rows]] @ (weights[s].t() if transpose else weights[s]))
    return out if bias is None else out + bias


class _RoundBf16(torch.autograd.Function):
    """x rounded to the nearest bf16 value, kept in its dtype; the gradient passes as it is"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _bf16_operands(operands):
    """Decided at the call, before .apply: custom_fwd turns autocast off inside the node."""
    if operands not in OPERANDS:
        raise ValueError("ao_amd octformer: operands must be one of %s, got %r" % (", ".join(map(repr, OPERANDS)), operands))
    return operands == "bf16" or (operands == "autocast" and torch.is_autocast_enabled("cuda"))


def octree_conv(x, weights, bias, table, form, operands="fp32"):
    """The dense octree convolutions of OctFormer's stem, Downsample and decoder on ao_amd/csrc/oct_conv.hip, one autograd node:
    form "conv3"    (n, Cout) from x (n, Cin), weights (27, Cin, Cout) and the OctreeLevel;
    form "down2"    (n_parent, Cout) from x (n, Cin), weights (8, Cin, Cout) and the OctreeLink;
    form "deconv3"  (n, Cout) from x (n_parent, Cin), weights (27, Cout, Cin) and the OctreeLink.
    fp32, under autocast too.  ValueError outside Cin % 4 == 0 (or Cin <= 8), Cout % 8 == 0, both at most 384.
    operands: "fp32" is that path whatever autocast says; "bf16" runs ao_amd/csrc/oct_conv_bf16.hip (x, W and the output's
    gradient rounded to bf16 on their way into the matrix core; accumulation, bias and everything in memory fp32); "autocast" is
    bf16 exactly when CUDA autocast is on at the call.  A stem layer (Cin <= 8) keeps the fp32 kernel whatever it says.  The
    eager path rounds x and W through bf16 (straight-through gradient; g is not rounded there) unless they are float64."""
    _lib.require_cuda(x, weights, bias)
    bf16 = _bf16_operands(operands)
    tab, transpose = conv_tables(table, form)[:2]
    n_in = table.n_parent if form == "deconv3" else table.n
    slots = tab.shape[1]
    if x.dim() != 2 or x.shape[0] != n_in or weights.dim() != 3 or weights.shape[0] != slots or weights.shape[2 if transpose else 1] != x.shape[1]:
        raise ValueError("ao_amd octformer: a %s takes x (%d, Cin) and weights (%d, %s); got %s %s"
                         % (form, n_in, slots, "Cout, Cin" if transpose else "Cin, Cout", tuple(x.shape), tuple(weights.shape)))
    cin, cout = x.shape[1], weights.shape[1 if transpose else 2]
    if not (1 <= cin <= CONV_STEM or (cin % 4 == 0 and cin <= CONV_MAX)):
        raise ValueError("ao_amd octformer: %d input channels; a multiple of 4 up to %d, or at most %d" % (cin, CONV_MAX, CONV_STEM))
    if cout % 8 or not 8 <= cout <= CONV_MAX:
        raise ValueError("ao_amd octformer: %d output channels; a multiple of 8, at most %d" % (cout, CONV_MAX))
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError("ao_amd octformer: bias is (%d,); got %s" % (cout, tuple(bias.shape)))
    bf16 = bf16 and cin > CONV_STEM
    if mode() == "torch":
        with torch.autocast("cuda", enabled=False):
            x, weights = _wide(x), _wide(weights)
            if bf16 and x.dtype != torch.float64:
                x, weights = _RoundBf16.apply(x), _RoundBf16.apply(weights)
            return octree_conv_torch(x, weights, None if bias is None else _wide(bias), tab, transpose)
    return _Conv.apply(x, weights, bias, table, form, cin, cout, bf16)


def octree_deconv(x, weights, link, operands="fp32"):
    """octree_conv's form "deconv3": the k = 3, stride 2 deconvolution from the parents to the children of `link`"""
    return octree_conv(x, weights, None, link, "deconv3", operands)
