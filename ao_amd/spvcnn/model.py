"""SPVCNN (the point-voxel network the reference drives with torchsparse) on the MI355X.

Reference: pointcept/models/spvcnn/ts_spvcnn.py.  Same constructor keywords and the same module tree (`stem`, `stage1..4`,
`up1..4`, `classifier`, `point_transforms`, `dropout`), so a torchsparse checkpoint's state dict loads by name and shape: every
convolution is a module whose one parameter is `kernel`, (K, Cin, Cout), or (Cin, Cout) for kernel_size 1, without a bias;
every norm carries nn.BatchNorm1d's keys.  The execution differs:

  * one PointVoxelMap per forward (ao_amd/spvcnn/pvmap.py) with one table build inside it serves every convolution and every
    point-voxel operator -- the reference hashes coordinates per stride as it meets them;
  * the voxel branch runs on the sparse convolutions of ao_amd/spunet/conv.py; `krsc_weight` is the one place where a kernel
    changes layout;
  * initial_voxelize / point_to_voxel / voxel_to_point are `voxelize` / `devoxelize` of ao_amd/spvcnn/ops.py; the sum
    `z.F = devoxelize(x) + point_transforms(z_prev.F)` is the `add` operand of the devoxelize kernel;
  * BatchNorm, ReLU and the residual tail are RowBatchNorm1d / bn_residual_relu (ao_amd/ptv2/layers.py); dropout is torch's.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..ptv2.layers import WGRAD_MIN_ROWS, RowBatchNorm1d, RowLinear, _LinearRows, bn_residual_relu
from ..spunet import conv
from ..spunet.model import SparseTensor
from .ops import devoxelize, voxelize
from .pvmap import LEVELS, point_voxel_map


def krsc_weight(kernel, kernel_size):
    """torchsparse's (K, Cin, Cout) kernel as the (Cout, k, k, k, Cin) weight of ao_amd/spunet/conv.py.
    k = 3: torchsparse numbers the kernel offsets with x fastest, include/ptv2_spconv_hip.h row-major with x slowest, so the
    three kernel axes are reversed; k = 2: the same order on both sides; k = 1 never comes here (a row GEMM)."""
    k, (_, cin, cout) = kernel_size, kernel.shape
    w = kernel.view(k, k, k, cin, cout)
    if k == 3:
        w = w.permute(2, 1, 0, 3, 4)
    return w.permute(4, 0, 1, 2, 3).contiguous()


class Conv3d(nn.Module):
    """spnn.Conv3d as ts_spvcnn.py uses it: kernel_size 3 / stride 1 (outputs at the input voxels), kernel_size 2 / stride 2
    (one level down), the same transposed (one level up), kernel_size 1 (rows)"""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, transposed=False):
        super().__init__()
        if (kernel_size, stride) not in ((3, 1), (2, 2), (1, 1)) or dilation != 1 or (transposed and kernel_size != 2):
            raise ValueError("ao_amd spvcnn: Conv3d is kernel_size 3 / stride 1, 2 / 2 (also transposed) or 1 / 1, dilation 1")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.transposed = stride, transposed
        volume = kernel_size ** 3
        self.kernel = nn.Parameter(torch.empty((volume, in_channels, out_channels) if volume > 1 else (in_channels, out_channels)))
        # torchsparse's own default: U(-s, s), s = 1 / sqrt((Cout if transposed else Cin) * K)
        bound = 1.0 / math.sqrt((out_channels if transposed else in_channels) * volume)
        nn.init.uniform_(self.kernel, -bound, bound)

    def forward(self, x):
        f = x.features
        if self.kernel_size == 1:
            _lib.require_cuda(f)
            w = self.kernel.t().contiguous()
            if (f.dtype == torch.float32 and f.shape[0] >= WGRAD_MIN_ROWS and torch.is_grad_enabled() and w.requires_grad
                    and self.in_channels % 4 == 0 and self.out_channels % 4 == 0):
                return x.replace_feature(_LinearRows.apply(f.contiguous(), w, None))
            return x.replace_feature(F.linear(f, w))
        w = krsc_weight(self.kernel, self.kernel_size)
        if self.kernel_size == 3:
            return x.replace_feature(conv.subm_conv(f, w, x.tables, x.level, 3))
        if self.transposed:
            if x.level < 1:
                raise ValueError("ao_amd spvcnn: a transposed convolution at level 0")
            return SparseTensor(conv.inverse_conv(f, w, x.tables, x.level - 1), x.tables, x.level - 1)
        if x.level + 1 >= LEVELS:
            raise ValueError("ao_amd spvcnn: at most %d downsamplings" % (LEVELS - 1))
        return SparseTensor(conv.down_conv(f, w, x.tables, x.level), x.tables, x.level + 1)

    def extra_repr(self):
        return "%d, %d, kernel_size=%d, stride=%d%s" % (self.in_channels, self.out_channels, self.kernel_size, self.stride,
                                                        ", transposed" if self.transposed else "")


def _conv_bn_relu(conv_, bn, x):
    y = conv_(x)
    return y.replace_feature(bn(y.features, relu=True))


class BasicConvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), RowBatchNorm1d(outc), nn.ReLU(True))

    def forward(self, x):
        return _conv_bn_relu(self.net[0], self.net[1], x)


class BasicDeconvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1):
        super().__init__()
        self.net = nn.Sequential(Conv3d(inc, outc, kernel_size=ks, stride=stride, transposed=True), RowBatchNorm1d(outc), nn.ReLU(True))

    def forward(self, x):
        return _conv_bn_relu(self.net[0], self.net[1], x)


class ResidualBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), RowBatchNorm1d(outc), nn.ReLU(True),
                                 Conv3d(outc, outc, kernel_size=ks, dilation=dilation, stride=1), RowBatchNorm1d(outc))
        if inc == outc and stride == 1:
            self.downsample = nn.Identity()
        else:
            self.downsample = nn.Sequential(Conv3d(inc, outc, kernel_size=1, dilation=1, stride=stride), RowBatchNorm1d(outc))
        self.relu = nn.ReLU(True)

    def forward(self, x):
        out = self.net[3](_conv_bn_relu(self.net[0], self.net[1], x))
        identity = x.features if isinstance(self.downsample, nn.Identity) else self.downsample[1](self.downsample[0](x).features)
        return out.replace_feature(bn_residual_relu(self.net[4], out.features, identity))  # relu(net(x) + downsample(x))


class _SparseBlocks(nn.Sequential):
    """nn.Sequential whose members take and return a SparseTensor (the same keys as the reference's nn.Sequential)"""


def _cat(a, b):
    return a.replace_feature(torch.cat((a.features, b.features), dim=1))  # torchsparse.cat


class SPVCNN(nn.Module):
    def __init__(self, in_channels, out_channels, base_channels=32, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                 layers=(2, 2, 2, 2, 2, 2, 2, 2)):
        super().__init__()
        assert len(layers) % 2 == 0
        assert len(layers) == len(channels)
        if len(layers) != 2 * (LEVELS - 1):
            raise ValueError("ao_amd spvcnn: %d stages (the reference's forward names stage1..4 and up1..4)" % (len(layers) // 2))
        self.in_channels, self.out_channels, self.base_channels = in_channels, out_channels, base_channels
        self.channels, self.layers = channels, layers
        self.num_stages = len(layers) // 2
        self.stem = nn.Sequential(Conv3d(in_channels, base_channels, kernel_size=3, stride=1), RowBatchNorm1d(base_channels), nn.ReLU(True),
                                  Conv3d(base_channels, base_channels, kernel_size=3, stride=1), RowBatchNorm1d(base_channels),
                                  nn.ReLU(True))
        widths = (base_channels,) + tuple(channels)
        for s in range(4):   # stage1..4: one level down, then layers[s] residual blocks
            inc, outc = widths[s], widths[s + 1]
            setattr(self, "stage%d" % (s + 1), _SparseBlocks(
                BasicConvolutionBlock(inc, inc, ks=2, stride=2, dilation=1), ResidualBlock(inc, outc, ks=3, stride=1, dilation=1),
                *[ResidualBlock(outc, outc, ks=3, stride=1, dilation=1) for _ in range(layers[s] - 1)]))
        for s in range(4):   # up1..4: one level up, the skip of that level, layers[4 + s] residual blocks
            inc, outc, skip = widths[4 + s], widths[5 + s], widths[3 - s]
            setattr(self, "up%d" % (s + 1), nn.ModuleList([
                BasicDeconvolutionBlock(inc, outc, ks=2, stride=2),
                _SparseBlocks(ResidualBlock(outc + skip, outc, ks=3, stride=1, dilation=1),
                              *[ResidualBlock(outc, outc, ks=3, stride=1, dilation=1) for _ in range(layers[4 + s] - 1)])]))
        self.classifier = nn.Sequential(RowLinear(channels[7], out_channels))
        self.point_transforms = nn.ModuleList([
            nn.Sequential(RowLinear(a, b), RowBatchNorm1d(b), nn.ReLU(True))
            for a, b in ((base_channels, channels[3]), (channels[3], channels[5]), (channels[5], channels[7]))])
        self.weight_initialization()
        self.dropout = nn.Dropout(0.3, True)

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _stem(self, x):
        return _conv_bn_relu(self.stem[3], self.stem[4], _conv_bn_relu(self.stem[0], self.stem[1], x))

    def _transform(self, which, feat):
        linear, bn, _ = self.point_transforms[which]
        return bn(linear(feat), relu=True)

    def forward(self, data_dict):
        discrete_coord, feat, offset = data_dict["discrete_coord"], data_dict["feat"], data_dict["offset"]
        _lib.require_cuda(discrete_coord, feat, offset)
        pv = point_voxel_map(discrete_coord, offset)  # THE map (and table) build of the forward
        sparse = lambda f, level: SparseTensor(f, pv.tables, level)  # noqa: E731

        x0 = self._stem(sparse(voxelize(feat, pv, 0), 0))                      # initial_voxelize, stem
        z0 = devoxelize(x0.features, pv, 0)                                    # voxel_to_point(x0, z)
        x1 = self.stage1(sparse(voxelize(z0, pv, 0), 0))                       # point_to_voxel(x0, z0)
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        z1 = devoxelize(x4.features, pv, 4, add=self._transform(0, z0))        # voxel_to_point(x4, z0) + point_transforms[0](z0.F)

        y1 = sparse(self.dropout(voxelize(z1, pv, 4)), 4)                      # point_to_voxel(x4, z1)
        y1 = self.up1[1](_cat(self.up1[0](y1), x3))
        y2 = self.up2[1](_cat(self.up2[0](y1), x2))
        z2 = devoxelize(y2.features, pv, 2, add=self._transform(1, z1))

        y3 = sparse(self.dropout(voxelize(z2, pv, 2)), 2)                      # point_to_voxel(y2, z2)
        y3 = self.up3[1](_cat(self.up3[0](y3), x1))
        y4 = self.up4[1](_cat(self.up4[0](y3), x0))
        z3 = devoxelize(y4.features, pv, 0, add=self._transform(2, z2))
        return self.classifier(z3)
