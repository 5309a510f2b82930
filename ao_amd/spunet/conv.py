"""The three convolutions of SpUNet-v1m1 as autograd nodes over the tables of ao_amd/spunet/tables.py.

A weight is (Cout, k, k, k, Cin) -- spconv.pytorch's KRSC layout -- read as (Cout, K, Cin); kappa is the row-major index of the
kernel offset along the three columns of discrete_coord:

    subm_conv      out[i]               = sum over kappa of W[kappa] in[nbr[i, kappa]]          SubMConv3d(k = 3 or 5)
    down_conv      out[o]               = sum over kappa of W[kappa] in[child[o, kappa]]        SparseConv3d(k = 2, stride = 2)
    inverse_conv   out[child[o, kappa]] = W[kappa] in[o]                                        SparseInverseConv3d(k = 2)

The HIP path is ao_amd/csrc/spconv.hip (C ABI: include/ptv2_spconv_hip.h): no (n, K, C) tensor exists in either direction, the
input gradient of a submanifold convolution reads its own table with the columns reversed (j = nbr[i, kappa] exactly when
i = nbr[j, K - 1 - kappa]), and every sum has a fixed order.  AO_AMD_SPUNET=torch runs each convolution as an eager loop over
kappa of index_select and matmul on the same tables (the A/B path of the parity tests).  There is no CPU fallback on either path.

operands="bf16" runs the matrix-core forms on ao_amd/csrc/spconv_bf16.hip (C ABI: include/ptv2_spconv_bf16_hip.h): both operands
of every product -- x and W, g and W, g and x -- are rounded to bf16 on their way into the matrix core, accumulation and
everything in memory stay fp32.  "autocast" means bf16 exactly when CUDA autocast is on at the call (float16 autocast too), as
the row GEMMs of ao_amd/ptv2 do; the default "fp32" is the exact path whatever autocast says.  The stem (Cin <= 16) has no
bf16 form and runs its fp32 kernel.  On the eager path bf16 operands round x and W through .bfloat16().float() first (g is not
rounded there).
"""
import os

import torch

from .. import _abi, _lib
from .tables import SpconvTables

_K = _abi.spconv_consts
GATHER, SCATTER = _K["SPCONV_GATHER"], _K["SPCONV_SCATTER"]
STEM_MAX_CIN = 16


def _use_hip():
    return os.environ.get("AO_AMD_SPUNET", "hip") != "torch"


# ------------------------------------------------------------------------------------------------------- eager torch -------
def gather_torch(x, tab, w):
    """out[r] = sum over kappa of in[tab[r, kappa]] W[kappa]^T; w (Cout, K, Cin)"""
    out = x.new_zeros((tab.shape[0], w.shape[0]))
    for kappa in range(tab.shape[1]):
        j = tab[:, kappa]
        rows = x.index_select(0, j.clamp(min=0).long()) * (j >= 0).unsqueeze(1).to(x.dtype)
        out = out + rows @ w[:, kappa].t()
    return out


def scatter_torch(x, tab, w, n_out):
    """out[tab[r, kappa]] = in[r] W[kappa]^T"""
    out = x.new_zeros((n_out, w.shape[0]))
    for kappa in range(tab.shape[1]):
        j = tab[:, kappa]
        rows = (x @ w[:, kappa].t()) * (j >= 0).unsqueeze(1).to(x.dtype)
        out = out.index_add(0, j.clamp(min=0).long(), rows)
    return out


# --------------------------------------------------------------------------------------------------------------- HIP -------
def _conv(form, x, tab, n_other, w, transpose, reverse, n_out, bf16=False):
    cout, k, cin = w.shape
    out = torch.empty((n_out, cin if transpose else cout), dtype=torch.float32, device=x.device)
    if bf16:
        L = _lib.lib()
        ws = _lib.workspace(L.ptv2_spconv_bf16_workspace_bytes(tab.shape[0], k, cin, cout), x.device)
        rc = L.spconv_bf16_conv_hip_launcher(form, tab.shape[0], n_other, k, cin, cout, x.data_ptr(), tab.data_ptr(), w.data_ptr(),
                                             int(transpose), int(reverse), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr())
        _lib.check(rc, "spconv_bf16_conv_hip_launcher")
        return out
    rc = _lib.lib().spconv_conv_hip_launcher(form, tab.shape[0], n_other, k, cin, cout, x.data_ptr(), tab.data_ptr(), w.data_ptr(),
                                             int(transpose), int(reverse), out.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "spconv_conv_hip_launcher")
    return out


def _stem(x, tab, w, transpose):
    cout, k, cin = w.shape
    out = torch.empty((tab.shape[0], cin if transpose else cout), dtype=torch.float32, device=x.device)
    rc = _lib.lib().spconv_stem_hip_launcher(tab.shape[0], k, cin, cout, x.data_ptr(), tab.data_ptr(), w.data_ptr(), int(transpose),
                                             out.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "spconv_stem_hip_launcher")
    return out


def _wgrad(x, g, tab, n_other, gather_g, w, bf16=False):
    cout, k, cin = w.shape
    L = _lib.lib()
    gw = torch.empty_like(w)
    if bf16:
        ws = _lib.workspace(L.ptv2_spconv_bf16_workspace_bytes(tab.shape[0], k, cin, cout), x.device)
        rc = L.spconv_bf16_wgrad_hip_launcher(tab.shape[0], n_other, k, cin, cout, x.data_ptr(), g.data_ptr(), tab.data_ptr(),
                                              int(gather_g), gw.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "spconv_bf16_wgrad_hip_launcher")
        return gw
    ws = _lib.workspace(L.ptv2_spconv_workspace_bytes(tab.shape[0], k, cin, cout), x.device)
    rc = L.spconv_wgrad_hip_launcher(tab.shape[0], n_other, k, cin, cout, x.data_ptr(), g.data_ptr(), tab.data_ptr(), int(gather_g),
                                     gw.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "spconv_wgrad_hip_launcher")
    return gw


class _SubM(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, tab, bf16):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, tab)
        ctx.bf16 = bf16  # (never set for the stem: _run)
        if w.shape[2] <= STEM_MAX_CIN:
            return _stem(x, tab, w, False)
        return _conv(GATHER, x, tab, x.shape[0], w, False, False, tab.shape[0], bf16)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, tab = ctx.saved_tensors
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gx = (_stem(g, tab, w, True) if w.shape[2] <= STEM_MAX_CIN
                  else _conv(GATHER, g, tab, x.shape[0], w, True, True, x.shape[0], ctx.bf16))
        gw = _wgrad(x, g, tab, x.shape[0], False, w, ctx.bf16) if ctx.needs_input_grad[1] else None
        return gx, gw, None, None


class _Down(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, child, bf16):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, child)
        ctx.bf16 = bf16
        return _conv(GATHER, x, child, x.shape[0], w, False, False, child.shape[0], bf16)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, child = ctx.saved_tensors
        g = g.contiguous()
        gx = _conv(SCATTER, g, child, x.shape[0], w, True, False, x.shape[0], ctx.bf16) if ctx.needs_input_grad[0] else None
        gw = _wgrad(x, g, child, x.shape[0], False, w, ctx.bf16) if ctx.needs_input_grad[1] else None
        return gx, gw, None, None


class _Inverse(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, child, n_fine, bf16):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, child)
        ctx.n_fine, ctx.bf16 = n_fine, bf16
        return _conv(SCATTER, x, child, n_fine, w, False, False, n_fine, bf16)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, child = ctx.saved_tensors
        g = g.contiguous()
        gx = _conv(GATHER, g, child, ctx.n_fine, w, True, False, x.shape[0], ctx.bf16) if ctx.needs_input_grad[0] else None
        gw = _wgrad(x, g, child, ctx.n_fine, True, w, ctx.bf16) if ctx.needs_input_grad[1] else None
        return gx, gw, None, None, None


# ------------------------------------------------------------------------------------------------------------ public -------
def _tables(tables, what):
    if not isinstance(tables, SpconvTables):
        raise TypeError("ao_amd spunet: %s takes the SpconvTables of build_tables(), not %s" % (what, type(tables).__name__))
    return tables


def _check(x, weight, tables, rows, k, what):
    _lib.require_cuda(x, weight)
    if weight.dim() != 5 or tuple(weight.shape[1:4]) != (k, k, k):
        raise ValueError("ao_amd spunet: %s weight must be (Cout, %d, %d, %d, Cin), got %s" % (what, k, k, k, tuple(weight.shape)))
    cout, cin = weight.shape[0], weight.shape[4]
    if x.dim() != 2 or tuple(x.shape) != (rows, cin):
        raise ValueError("ao_amd spunet: %s input must be (%d, %d), got %s" % (what, rows, cin, tuple(x.shape)))
    return weight.reshape(cout, k * k * k, cin)


def _widths_ok(w, stem):
    cout, _, cin = w.shape
    if stem and cin <= STEM_MAX_CIN:
        return cout in (32, 64) and w.shape[1] * cin * cout * 4 <= 147456
    return cin % 32 == 0 and cout % 32 == 0


OPERANDS = ("fp32", "bf16", "autocast")


def _bf16_operands(operands):
    """Decided at the call, before .apply: custom_fwd turns autocast off inside the node."""
    if operands not in OPERANDS:
        raise ValueError("ao_amd spunet: operands must be one of %s, got %r" % (", ".join(map(repr, OPERANDS)), operands))
    return operands == "bf16" or (operands == "autocast" and torch.is_autocast_enabled("cuda"))


class _RoundBf16(torch.autograd.Function):
    """x rounded to the nearest bf16 value, kept in fp32; the gradient passes as it is"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g


def _run(node, torch_fn, x, w, stem, operands, *args):
    bf16 = _bf16_operands(operands) and not (stem and w.shape[2] <= STEM_MAX_CIN)
    if not _use_hip():
        with torch.autocast("cuda", enabled=False):
            x, w = x.float(), w.float()
            if bf16:
                x, w = _RoundBf16.apply(x), _RoundBf16.apply(w)
            return torch_fn(x, w)
    if not _widths_ok(w, stem):  # a missing kernel is an error, not a fall-back
        raise ValueError("ao_amd spunet: no kernel for Cin = %d, Cout = %d (multiples of 32; the stem: Cin <= %d, Cout 32 or 64)"
                         % (w.shape[2], w.shape[0], STEM_MAX_CIN))
    return node.apply(x, w, *args, bf16)


def subm_conv(x, weight, tables, level, kernel_size=3, operands="fp32"):
    """SubMConv3d(kernel_size 3 at any level, 5 at level 0): x (n_level, Cin) -> (n_level, Cout).  operands: "fp32", "bf16"
    or "autocast" (the module docstring); the stem form (Cin <= 16) runs its fp32 kernel whatever it says."""
    if kernel_size not in (3, 5) or (kernel_size == 5 and level != 0):
        raise ValueError("ao_amd spunet: submanifold kernels are 3 (any level) and 5 (level 0)")
    w = _check(x, weight, tables, _tables(tables, "subm_conv").n[level], kernel_size, "subm_conv")
    tab = tables.nbr5 if kernel_size == 5 else tables.nbr3[level]
    return _run(_SubM, lambda a, b: gather_torch(a, tab, b), x, w, True, operands, tab)


def down_conv(x, weight, tables, level, operands="fp32"):
    """SparseConv3d(kernel_size 2, stride 2) from `level` to level + 1: x (n_level, Cin) -> (n_{level + 1}, Cout)"""
    w = _check(x, weight, tables, _tables(tables, "down_conv").n[level], 2, "down_conv")
    tab = tables.child[level]
    return _run(_Down, lambda a, b: gather_torch(a, tab, b), x, w, False, operands, tab)


def inverse_conv(x, weight, tables, level, operands="fp32"):
    """SparseInverseConv3d(kernel_size 2) from level + 1 back to `level`: x (n_{level + 1}, Cin) -> (n_level, Cout)"""
    w = _check(x, weight, tables, _tables(tables, "inverse_conv").n[level + 1], 2, "inverse_conv")
    tab, n_fine = tables.child[level], tables.n[level]
    return _run(_Inverse, lambda a, b: scatter_torch(a, tab, b, n_fine), x, w, False, operands, tab, n_fine)
