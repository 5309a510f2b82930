"""SpUNet-v1m1 (the sparse U-Net the reference drives with spconv) on the MI355X.

Reference: pointcept/models/sparse_unet/spconv_unet_v1m1_base.py.  Same constructor keywords, same state-dict keys and shapes
(`load_state_dict(strict=True)` works in both directions; a convolution's weight is (Cout, k, k, k, Cin), spconv.pytorch's
KRSC layout); the execution differs:

  * one table build per forward (ao_amd/spunet/tables.py) serves every convolution of the encoder and the decoder -- spconv
    builds a table per `indice_key` as it meets it -- with one host read-back;
  * the three convolutions are autograd nodes on ao_amd/csrc/spconv.hip (ao_amd/spunet/conv.py) and never form an (n, K, C)
    tensor; the 1 x 1 x 1 convolutions (BasicBlock.proj, final) are row Linears on a view of their five-dimensional weight;
  * BatchNorm, ReLU and the residual tail are RowBatchNorm1d / bn_residual_relu (ao_amd/ptv2/layers.py);
  * every sum has a fixed order: two identical steps give the same bits.

`cls_mode=True` is not implemented.  fp32 only: under torch.autocast the nodes take fp32 inputs.
"""
import math
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..ptv2.layers import WGRAD_MIN_ROWS, RowBatchNorm1d, _LinearRows, bn_residual_relu
from . import conv
from .tables import LEVELS, build_tables


class SparseTensor:
    """features (n_level, C) of one level of a batch's tables (what spconv.SparseConvTensor is to the reference's modules)"""

    def __init__(self, features, tables, level=0):
        self.features, self.tables, self.level = features, tables, level

    def replace_feature(self, features):
        return SparseTensor(features, self.tables, self.level)


class _SparseConv(nn.Module):
    kind = None

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False, indice_key=None):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.indice_key = stride, padding, indice_key
        k = kernel_size
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # spconv's own default (kaiming_uniform with a = sqrt(5) over fan_in = k^3 Cin): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        bound = 1.0 / math.sqrt(self.kernel_size ** 3 * self.in_channels)
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    def _table(self, x):
        kind, level = x.tables.lookup(self.indice_key, x.level, self.kernel_size)
        if kind != self.kind:
            raise ValueError("ao_amd spunet: indice_key %r names a %s table, the module needs %s" % (self.indice_key, kind, self.kind))
        return level

    def _add_bias(self, y):
        return y if self.bias is None else y + self.bias.to(y.dtype)

    def extra_repr(self):
        return "%d, %d, kernel_size=%d, stride=%d, indice_key=%r" % (self.in_channels, self.out_channels, self.kernel_size,
                                                                     self.stride, self.indice_key)


class SubMConv3d(_SparseConv):
    """Outputs at the input voxels, in input order; the kernel is centred whatever `padding` says.  kernel_size 1 is a row
    Linear on the (Cout, Cin) view of the weight."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False, indice_key=None):
        if kernel_size not in (1, 3, 5):
            raise ValueError("ao_amd spunet: SubMConv3d kernel sizes are 1, 3 and 5")
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, indice_key)
        self.kind = "subm5" if kernel_size == 5 else "subm3"

    def forward(self, x):
        f = x.features
        if self.kernel_size == 1:
            _lib.require_cuda(f)
            w = self.weight.view(self.out_channels, self.in_channels)
            if (f.dtype == torch.float32 and f.shape[0] >= WGRAD_MIN_ROWS and torch.is_grad_enabled() and w.requires_grad
                    and self.in_channels % 4 == 0 and self.out_channels % 4 == 0):
                return x.replace_feature(_LinearRows.apply(f.contiguous(), w, self.bias))
            return x.replace_feature(F.linear(f, w, self.bias))
        level = self._table(x)
        if level != x.level:
            raise ValueError("ao_amd spunet: indice_key %r is level %d, the input is level %d" % (self.indice_key, level, x.level))
        return x.replace_feature(self._add_bias(conv.subm_conv(f, self.weight, x.tables, level, self.kernel_size)))


class SparseConv3d(_SparseConv):
    """kernel_size 2, stride 2: one output per occupied coarse voxel coord >> 1, in ascending (cloud, x, y, z) order"""
    kind = "down"

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False, indice_key=None):
        if kernel_size != 2 or stride != 2:
            raise ValueError("ao_amd spunet: SparseConv3d is kernel_size 2, stride 2")
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, indice_key)

    def forward(self, x):
        level = x.level if self.indice_key is None else self._table(x)
        if level != x.level or level + 1 >= LEVELS:
            raise ValueError("ao_amd spunet: indice_key %r downsamples level %d, the input is level %d" % (self.indice_key, level, x.level))
        y = conv.down_conv(x.features, self.weight, x.tables, level)
        return SparseTensor(self._add_bias(y), x.tables, level + 1)


class SparseInverseConv3d(_SparseConv):
    """kernel_size 2: the table of the SparseConv3d with the same indice_key, the other way"""
    kind = "down"

    def __init__(self, in_channels, out_channels, kernel_size, bias=False, indice_key=None):
        if kernel_size != 2:
            raise ValueError("ao_amd spunet: SparseInverseConv3d is kernel_size 2")
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, indice_key)

    def forward(self, x):
        level = x.level - 1 if self.indice_key is None else self._table(x)
        if level != x.level - 1 or level < 0:
            raise ValueError("ao_amd spunet: indice_key %r leads back to level %d, the input is level %d" % (self.indice_key, level, x.level))
        y = conv.inverse_conv(x.features, self.weight, x.tables, level)
        return SparseTensor(self._add_bias(y), x.tables, level)


class SparseSequential(nn.Sequential):
    """nn.Sequential over SparseTensor: a module that is not a sparse one acts on the features (a norm followed by nn.ReLU
    runs as one fused pass)"""

    def forward(self, x):
        mods = list(self)
        at = 0
        while at < len(mods):
            m = mods[at]
            if isinstance(m, (_SparseConv, SparseSequential, BasicBlock)):
                x = m(x)
            elif isinstance(m, RowBatchNorm1d) and at + 1 < len(mods) and isinstance(mods[at + 1], nn.ReLU):
                x = x.replace_feature(m(x.features, relu=True))
                at += 1
            else:
                x = x.replace_feature(m(x.features))
            at += 1
        return x


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        assert norm_fn is not None
        if in_channels == embed_channels:
            self.proj = SparseSequential(nn.Identity())
        else:
            self.proj = SparseSequential(SubMConv3d(in_channels, embed_channels, kernel_size=1, bias=False), norm_fn(embed_channels))
        self.conv1 = SubMConv3d(in_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(embed_channels)
        self.relu = nn.ReLU()
        self.conv2 = SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                indice_key=indice_key)
        self.bn2 = norm_fn(embed_channels)
        self.stride = stride

    def forward(self, x):
        out = self.conv1(x)
        out = out.replace_feature(self.bn1(out.features, relu=True))
        out = self.conv2(out)
        return out.replace_feature(bn_residual_relu(self.bn2, out.features, self.proj(x).features))


def _norm(channels):
    return RowBatchNorm1d(channels, eps=1e-3, momentum=0.01)


class SpUNetBase(nn.Module):
    def __init__(self, in_channels, num_classes, base_channels=32, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                 layers=(2, 3, 4, 6, 2, 2, 2, 2), cls_mode=False):
        super().__init__()
        assert len(layers) % 2 == 0
        assert len(layers) == len(channels)
        if cls_mode:
            raise NotImplementedError("ao_amd spunet: cls_mode is not implemented")
        self.in_channels, self.num_classes, self.base_channels = in_channels, num_classes, base_channels
        self.channels, self.layers = channels, layers
        self.num_stages = len(layers) // 2
        self.cls_mode = cls_mode
        if self.num_stages > LEVELS - 1:
            raise ValueError("ao_amd spunet: at most %d stages (include/ptv2_spconv_hip.h: SPCONV_LEVELS)" % (LEVELS - 1))
        norm_fn, block = _norm, BasicBlock
        self.conv_input = SparseSequential(
            SubMConv3d(in_channels, base_channels, kernel_size=5, padding=1, bias=False, indice_key="stem"),
            norm_fn(base_channels), nn.ReLU())
        enc_channels, dec_channels = base_channels, channels[-1]
        self.down, self.up, self.enc, self.dec = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for s in range(self.num_stages):
            self.down.append(SparseSequential(
                SparseConv3d(enc_channels, channels[s], kernel_size=2, stride=2, bias=False, indice_key="spconv%d" % (s + 1)),
                norm_fn(channels[s]), nn.ReLU()))
            self.enc.append(SparseSequential(OrderedDict(
                ("block%d" % i, block(channels[s], channels[s], norm_fn=norm_fn, indice_key="subm%d" % (s + 1)))
                for i in range(layers[s]))))
            self.up.append(SparseSequential(
                SparseInverseConv3d(channels[len(channels) - s - 2], dec_channels, kernel_size=2, bias=False,
                                    indice_key="spconv%d" % (s + 1)),
                norm_fn(dec_channels), nn.ReLU()))
            self.dec.append(SparseSequential(OrderedDict(
                ("block%d" % i, block(dec_channels + enc_channels if i == 0 else dec_channels, dec_channels, norm_fn=norm_fn,
                                      indice_key="subm%d" % s))
                for i in range(layers[len(channels) - s - 1]))))
            enc_channels = channels[s]
            dec_channels = channels[len(channels) - s - 2]
        self.final = (SubMConv3d(channels[-1], num_classes, kernel_size=1, padding=1, bias=True) if num_classes > 0
                      else nn.Identity())
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Linear, SubMConv3d)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, input_dict):
        discrete_coord, feat, offset = input_dict["discrete_coord"], input_dict["feat"], input_dict["offset"]
        _lib.require_cuda(discrete_coord, feat, offset)
        x = SparseTensor(feat, build_tables(discrete_coord, offset), 0)  # THE table build of the forward
        x = self.conv_input(x)
        skips = [x]
        for s in range(self.num_stages):
            x = self.enc[s](self.down[s](x))
            skips.append(x)
        x = skips.pop(-1)
        for s in reversed(range(self.num_stages)):
            x = self.up[s](x)
            skip = skips.pop(-1)
            x = x.replace_feature(torch.cat((x.features, skip.features), dim=1))
            x = self.dec[s](x)
        if self.num_classes > 0:
            x = self.final(x)
        return x.features
