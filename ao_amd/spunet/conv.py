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
def _conv(form, x, tab, n_other, w, transpose, reverse, n_out):
    cout, k, cin = w.shape
    out = torch.empty((n_out, cin if transpose else cout), dtype=torch.float32, device=x.device)
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


def _wgrad(x, g, tab, n_other, gather_g, w):
    cout, k, cin = w.shape
    L = _lib.lib()
    gw = torch.empty_like(w)
    ws = _lib.workspace(L.ptv2_spconv_workspace_bytes(tab.shape[0], k, cin, cout), x.device)
    rc = L.spconv_wgrad_hip_launcher(tab.shape[0], n_other, k, cin, cout, x.data_ptr(), g.data_ptr(), tab.data_ptr(), int(gather_g),
                                     gw.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "spconv_wgrad_hip_launcher")
    return gw


class _SubM(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, tab):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, tab)
        if w.shape[2] <= STEM_MAX_CIN:
            return _stem(x, tab, w, False)
        return _conv(GATHER, x, tab, x.shape[0], w, False, False, tab.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, tab = ctx.saved_tensors
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _stem(g, tab, w, True) if w.shape[2] <= STEM_MAX_CIN else _conv(GATHER, g, tab, x.shape[0], w, True, True, x.shape[0])
        gw = _wgrad(x, g, tab, x.shape[0], False, w) if ctx.needs_input_grad[1] else None
        return gx, gw, None


class _Down(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, child):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, child)
        return _conv(GATHER, x, child, x.shape[0], w, False, False, child.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, child = ctx.saved_tensors
        g = g.contiguous()
        gx = _conv(SCATTER, g, child, x.shape[0], w, True, False, x.shape[0]) if ctx.needs_input_grad[0] else None
        gw = _wgrad(x, g, child, x.shape[0], False, w) if ctx.needs_input_grad[1] else None
        return gx, gw, None


class _Inverse(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, child, n_fine):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w, child)
        ctx.n_fine = n_fine
        return _conv(SCATTER, x, child, n_fine, w, False, False, n_fine)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, w, child = ctx.saved_tensors
        g = g.contiguous()
        gx = _conv(GATHER, g, child, ctx.n_fine, w, True, False, x.shape[0]) if ctx.needs_input_grad[0] else None
        gw = _wgrad(x, g, child, ctx.n_fine, True, w) if ctx.needs_input_grad[1] else None
        return gx, gw, None, None


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


def _run(node, torch_fn, x, w, stem, *args):
    if not _use_hip():
        with torch.autocast("cuda", enabled=False):
            return torch_fn(x.float(), w.float())
    if not _widths_ok(w, stem):  # a missing kernel is an error, not a fall-back
        raise ValueError("ao_amd spunet: no kernel for Cin = %d, Cout = %d (multiples of 32; the stem: Cin <= %d, Cout 32 or 64)"
                         % (w.shape[2], w.shape[0], STEM_MAX_CIN))
    return node.apply(x, w, *args)


def subm_conv(x, weight, tables, level, kernel_size=3):
    """SubMConv3d(kernel_size 3 at any level, 5 at level 0): x (n_level, Cin) -> (n_level, Cout)"""
    if kernel_size not in (3, 5) or (kernel_size == 5 and level != 0):
        raise ValueError("ao_amd spunet: submanifold kernels are 3 (any level) and 5 (level 0)")
    w = _check(x, weight, tables, _tables(tables, "subm_conv").n[level], kernel_size, "subm_conv")
    tab = tables.nbr5 if kernel_size == 5 else tables.nbr3[level]
    return _run(_SubM, lambda a, b: gather_torch(a, tab, b), x, w, True, tab)


def down_conv(x, weight, tables, level):
    """SparseConv3d(kernel_size 2, stride 2) from `level` to level + 1: x (n_level, Cin) -> (n_{level + 1}, Cout)"""
    w = _check(x, weight, tables, _tables(tables, "down_conv").n[level], 2, "down_conv")
    tab = tables.child[level]
    return _run(_Down, lambda a, b: gather_torch(a, tab, b), x, w, False, tab)


def inverse_conv(x, weight, tables, level):
    """SparseInverseConv3d(kernel_size 2) from level + 1 back to `level`: x (n_{level + 1}, Cin) -> (n_level, Cout)"""
    w = _check(x, weight, tables, _tables(tables, "inverse_conv").n[level + 1], 2, "inverse_conv")
    tab, n_fine = tables.child[level], tables.n[level]
    return _run(_Inverse, lambda a, b: scatter_torch(a, tab, b, n_fine), x, w, False, tab, n_fine)
