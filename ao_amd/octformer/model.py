"""OctFormer's blocks of one depth (pointcept/models/octformer/octformer_v1m1_base.py:102-365 of the reference) with the
reference's constructor arguments and state-dict keys, on the operators of ops.py.

forward(data, level): `level` is the OctreeLevel of octree_level() and replaces the reference's (octree, depth) pair; `data` is
(n, C) in the order of `level`.  The Linears, LayerNorm, the GELU MLP, BatchNorm1d and the residuals stay torch.

The rest of the model (:368-615): PatchEmbed, Downsample, OctFormerDecoder and OctFormer on octree_conv of
ops.py, with ocnn's module and parameter names restated so that a reference checkpoint loads with strict=True.
"""
from typing import List, Optional

import torch
from torch.utils.checkpoint import checkpoint

from .octree import octree_pyramid
from .ops import OPERANDS, octree_attention, octree_conv, octree_dwconv, pos_bnd_of


class MLP(torch.nn.Module):
    def __init__(self, in_features: int, hidden_features: Optional[int] = None, out_features: Optional[int] = None,
                 activation=torch.nn.GELU, drop: float = 0.0, **kwargs):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features or in_features
        self.hidden_features = hidden_features or in_features
        self.fc1 = torch.nn.Linear(self.in_features, self.hidden_features)
        self.act = activation()
        self.fc2 = torch.nn.Linear(self.hidden_features, self.out_features)
        self.drop = torch.nn.Dropout(drop, inplace=True)

    def forward(self, data: torch.Tensor):
        data = self.drop(self.act(self.fc1(data)))
        return self.drop(self.fc2(data))


class OctreeDWConv(torch.nn.Module):
    """the depthwise 3 x 3 x 3 octree convolution; `weights` (27, 1, C) is ocnn's shape and key, restated from its
    documentation (unpinned)"""

    def __init__(self, in_channels: int, kernel_size: List[int] = [3], nempty: bool = False, use_bias: bool = False):
        super().__init__()
        if list(kernel_size) not in ([3], [3, 3, 3]) or use_bias:
            raise NotImplementedError("ao_amd octformer: OctreeDWConv with kernel_size [3] and no bias")
        self.in_channels = in_channels
        self.weights = torch.nn.Parameter(torch.empty(27, 1, in_channels))
        torch.nn.init.xavier_uniform_(self.weights)

    def forward(self, data: torch.Tensor, level):
        return octree_dwconv(data, self.weights, level)


class OctreeDWConvBn(torch.nn.Module):
    def __init__(self, in_channels: int, kernel_size: List[int] = [3], stride: int = 1, nempty: bool = False):
        super().__init__()
        self.conv = OctreeDWConv(in_channels, kernel_size, nempty, use_bias=False)
        self.bn = torch.nn.BatchNorm1d(in_channels)

    def forward(self, data: torch.Tensor, level):
        return self.bn(self.conv(data, level))


class RPE(torch.nn.Module):
    """holds the table; octree_attention reads it (the (P, K, K, 3) index gather of the reference's forward never exists)"""

    def __init__(self, patch_size: int, num_heads: int, dilation: int = 1):
        super().__init__()
        self.patch_size = patch_size
        self.num_heads = num_heads
        self.dilation = dilation
        self.pos_bnd = self.get_pos_bnd(patch_size)
        self.rpe_num = 2 * self.pos_bnd + 1
        self.rpe_table = torch.nn.Parameter(torch.zeros(3 * self.rpe_num, num_heads))
        torch.nn.init.trunc_normal_(self.rpe_table, std=0.02)

    def get_pos_bnd(self, patch_size: int):
        return pos_bnd_of(patch_size, self.dilation)

    def extra_repr(self) -> str:
        return "num_heads={}, pos_bnd={}, dilation={}".format(self.num_heads, self.pos_bnd, self.dilation)


class OctreeAttention(torch.nn.Module):
    def __init__(self, dim: int, patch_size: int, num_heads: int, qkv_bias: bool = True, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, dilation: int = 1, use_rpe: bool = True):
        super().__init__()
        if attn_drop or proj_drop:
            raise NotImplementedError("ao_amd octformer: attn_drop / proj_drop other than 0 (the reference config uses 0)")
        if not use_rpe:
            raise NotImplementedError("ao_amd octformer: use_rpe=False")
        self.dim = dim
        self.patch_size = patch_size
        self.num_heads = num_heads
        self.dilation = dilation
        self.use_rpe = use_rpe
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = torch.nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = torch.nn.Linear(dim, dim)
        self.rpe = RPE(patch_size, num_heads, dilation)

    def forward(self, data: torch.Tensor, level):
        data = octree_attention(self.qkv(data), level, self.rpe.rpe_table, self.patch_size, self.dilation, self.scale)
        return self.proj(data)

    def extra_repr(self) -> str:
        return "dim={}, patch_size={}, num_heads={}, dilation={}".format(self.dim, self.patch_size, self.num_heads, self.dilation)


class OctreeDropPath(torch.nn.Module):
    """one Bernoulli keep per cloud, scaled by 1 / keep_prob; the identity in eval or at rate 0"""

    def __init__(self, drop_prob: float = 0.0, nempty: bool = False, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, data: torch.Tensor, level):
        if self.drop_prob <= 0.0 or not self.training:
            return data
        keep_prob = 1 - self.drop_prob
        keep = torch.floor(torch.rand(level.clouds, 1, dtype=data.dtype, device=data.device) + keep_prob)
        if keep_prob > 0.0 and self.scale_by_keep:
            keep = keep / keep_prob
        return data * keep[level.batch.long()]


class OctFormerBlock(torch.nn.Module):
    def __init__(self, dim: int, num_heads: int, patch_size: int = 32, dilation: int = 0, mlp_ratio: float = 4.0,
                 qkv_bias: bool = True, qk_scale: Optional[float] = None, attn_drop: float = 0.0, proj_drop: float = 0.0,
                 drop_path: float = 0.0, nempty: bool = True, activation: torch.nn.Module = torch.nn.GELU, **kwargs):
        super().__init__()
        self.norm1 = torch.nn.LayerNorm(dim)
        self.attention = OctreeAttention(dim, patch_size, num_heads, qkv_bias, qk_scale, attn_drop, proj_drop, dilation)
        self.norm2 = torch.nn.LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * mlp_ratio), dim, activation, proj_drop)
        self.drop_path = OctreeDropPath(drop_path, nempty)
        self.cpe = OctreeDWConvBn(dim, nempty=nempty)

    def forward(self, data: torch.Tensor, level):
        data = self.cpe(data, level) + data
        attn = self.attention(self.norm1(data), level)
        data = data + self.drop_path(attn, level)
        ffn = self.mlp(self.norm2(data))
        data = data + self.drop_path(ffn, level)
        return data


class OctFormerStage(torch.nn.Module):
    def __init__(self, dim: int, num_heads: int, patch_size: int = 32, dilation: int = 0, mlp_ratio: float = 4.0,
                 qkv_bias: bool = True, qk_scale: Optional[float] = None, attn_drop: float = 0.0, proj_drop: float = 0.0,
                 drop_path: float = 0.0, nempty: bool = True, activation: torch.nn.Module = torch.nn.GELU, interval: int = 6,
                 use_checkpoint: bool = True, num_blocks: int = 2, octformer_block=OctFormerBlock, **kwargs):
        super().__init__()
        self.num_blocks = num_blocks
        self.use_checkpoint = use_checkpoint
        self.interval = interval
        self.num_norms = (num_blocks - 1) // self.interval
        self.blocks = torch.nn.ModuleList([
            octformer_block(dim=dim, num_heads=num_heads, patch_size=patch_size, dilation=1 if (i % 2 == 0) else dilation,
                            mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop,
                            drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, nempty=nempty,
                            activation=activation)
            for i in range(num_blocks)])

    def forward(self, data: torch.Tensor, level):
        for i in range(self.num_blocks):
            if self.use_checkpoint and self.training:
                data = checkpoint(self.blocks[i], data, level, use_reentrant=False)
            else:
                data = self.blocks[i](data, level)
        return data


# ------------------------------------------------------ the stem, Downsample, the decoder, the model ----
# forward(data, octree, depth): `octree` is the OctreePyramid of octree_pyramid(), `depth` the depth of `data`'s rows.
def _nempty(nempty):
    if not nempty:
        raise NotImplementedError("ao_amd octformer: nempty=False (the reference config builds every module with nempty=True)")


class OctreeConv(torch.nn.Module):
    """ocnn.nn.OctreeConv for kernel_size [3] with stride 1 and [2] with stride 2; `weights` (kdim, Cin, Cout) and `bias` are
    ocnn's shapes and keys, restated from its documentation (unpinned)"""
    transposed = False
    operands = "fp32"   # of octree_conv; PatchEmbed, Downsample and OctFormerDecoder set it from their conv_operands

    def __init__(self, in_channels: int, out_channels: int, kernel_size: List[int] = [3], stride: int = 1, nempty: bool = False,
                 direct_method: bool = False, use_bias: bool = False, max_buffer: int = int(2e8)):
        super().__init__()
        _nempty(nempty)
        k = [int(v) for v in kernel_size] * (3 if len(kernel_size) == 1 else 1)
        if (k, stride) not in (([3, 3, 3], 1), ([2, 2, 2], 2), ([3, 3, 3], 2)) or ((k, stride) == ([3, 3, 3], 2)) != self.transposed:
            raise NotImplementedError("ao_amd octformer: %s with kernel_size %s, stride %d" % (type(self).__name__, list(kernel_size), stride))
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, out_channels, k, stride
        self.form = "deconv3" if self.transposed else "conv3" if stride == 1 else "down2"
        kdim = k[0] ** 3
        self.weights = torch.nn.Parameter(torch.empty((kdim, out_channels, in_channels) if self.transposed else (kdim, in_channels, out_channels)))
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if use_bias else None
        torch.nn.init.xavier_uniform_(self.weights)

    def forward(self, data: torch.Tensor, octree, depth: int):
        table = octree.level(depth) if self.form == "conv3" else octree.link(depth if self.form == "down2" else depth + 1)
        return octree_conv(data, self.weights, self.bias, table, self.form, self.operands)

    def extra_repr(self) -> str:
        return "in_channels={}, out_channels={}, kernel_size={}, stride={}, bias={}".format(
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.bias is not None)


class OctreeDeconv(OctreeConv):
    """ocnn.nn.OctreeDeconv for kernel_size [3], stride 2: depth -> depth + 1; `weights` (27, Cout, Cin)"""
    transposed = True


def _set_conv_operands(module, conv_operands):
    """hands `conv_operands` ("fp32", "bf16" or "autocast") to every octree convolution below `module`"""
    if conv_operands not in OPERANDS:
        raise ValueError("ao_amd octformer: conv_operands must be one of %s, got %r" % (", ".join(map(repr, OPERANDS)), conv_operands))
    for m in module.modules():
        if isinstance(m, OctreeConv):
            m.operands = conv_operands


class OctreeConvBnRelu(torch.nn.Module):
    """ocnn.modules.OctreeConvBnRelu: `.conv`, `.bn` (eps 1e-5, momentum 0.01: ocnn.modules' defaults, restated), ReLU"""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: List[int] = [3], stride: int = 1, nempty: bool = False):
        super().__init__()
        self.conv = OctreeConv(in_channels, out_channels, kernel_size, stride, nempty)
        self.bn = torch.nn.BatchNorm1d(out_channels, eps=1e-5, momentum=0.01)
        self.relu = torch.nn.ReLU(inplace=True)

    def forward(self, data: torch.Tensor, octree, depth: int):
        return self.relu(self.bn(self.conv(data, octree, depth)))


class OctreeDeconvBnRelu(torch.nn.Module):
    """ocnn.modules.OctreeDeconvBnRelu: `.deconv`, `.bn`, ReLU"""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: List[int] = [3], stride: int = 1, nempty: bool = False):
        super().__init__()
        self.deconv = OctreeDeconv(in_channels, out_channels, kernel_size, stride, nempty)
        self.bn = torch.nn.BatchNorm1d(out_channels, eps=1e-5, momentum=0.01)
        self.relu = torch.nn.ReLU(inplace=True)

    def forward(self, data: torch.Tensor, octree, depth: int):
        return self.relu(self.bn(self.deconv(data, octree, depth)))


class OctreeUpsample(torch.nn.Module):
    """ocnn.nn.OctreeUpsample("nearest"): every child takes its parent's row, one depth after the other up to target_depth
    (torch indexing; its backward is an index_add)"""

    def __init__(self, method: str = "nearest", nempty: bool = False):
        super().__init__()
        _nempty(nempty)
        if method != "nearest":
            raise NotImplementedError("ao_amd octformer: OctreeUpsample(%r); nearest" % method)

    def forward(self, data: torch.Tensor, octree, depth: int, target_depth: Optional[int] = None):
        for d in range(depth + 1, (depth + 1 if target_depth is None else target_depth) + 1):
            data = data[octree.link(d).parent.long()]
        return data


class OctFormerDecoder(torch.nn.Module):
    def __init__(self, channels: List[int], fpn_channel: int, nempty: bool, head_up: int = 1, conv_operands: str = "fp32"):
        super().__init__()
        self.head_up = head_up
        self.num_stages = len(channels)
        self.conv1x1 = torch.nn.ModuleList([torch.nn.Linear(channels[i], fpn_channel) for i in range(self.num_stages - 1, -1, -1)])
        self.upsample = OctreeUpsample("nearest", nempty)
        self.conv3x3 = torch.nn.ModuleList([OctreeConvBnRelu(fpn_channel, fpn_channel, kernel_size=[3], stride=1, nempty=nempty)
                                            for _ in range(self.num_stages)])
        self.up_conv = torch.nn.ModuleList([OctreeDeconvBnRelu(fpn_channel, fpn_channel, kernel_size=[3], stride=2, nempty=nempty)
                                            for _ in range(self.head_up)])
        _set_conv_operands(self, conv_operands)

    def forward(self, features, octree):
        depth = min(features.keys())
        depth_max = max(features.keys())
        assert self.num_stages == len(features)

        feature = self.conv1x1[0](features[depth])
        conv_out = self.conv3x3[0](feature, octree, depth)
        out = self.upsample(conv_out, octree, depth, depth_max)
        for i in range(1, self.num_stages):
            depth_i = depth + i
            feature = self.upsample(feature, octree, depth_i - 1)
            feature = self.conv1x1[i](features[depth_i]) + feature
            conv_out = self.conv3x3[i](feature, octree, depth_i)
            out = out + self.upsample(conv_out, octree, depth_i, depth_max)
        for i in range(self.head_up):
            out = self.up_conv[i](out, octree, depth_max + i)
        return out


class PatchEmbed(torch.nn.Module):
    def __init__(self, in_channels: int = 3, dim: int = 96, num_down: int = 2, nempty: bool = True, conv_operands: str = "fp32",
                 **kwargs):
        super().__init__()
        self.num_stages = num_down
        self.delta_depth = -num_down
        channels = [int(dim * 2 ** i) for i in range(-self.num_stages, 1)]
        self.convs = torch.nn.ModuleList([OctreeConvBnRelu(in_channels if i == 0 else channels[i], channels[i], kernel_size=[3],
                                                           stride=1, nempty=nempty) for i in range(self.num_stages)])
        self.downsamples = torch.nn.ModuleList([OctreeConvBnRelu(channels[i], channels[i + 1], kernel_size=[2], stride=2, nempty=nempty)
                                                for i in range(self.num_stages)])
        self.proj = OctreeConvBnRelu(channels[-1], dim, kernel_size=[3], stride=1, nempty=nempty)
        _set_conv_operands(self, conv_operands)

    def forward(self, data: torch.Tensor, octree, depth: int):
        for i in range(self.num_stages):
            depth_i = depth - i
            data = self.convs[i](data, octree, depth_i)
            data = self.downsamples[i](data, octree, depth_i)
        return self.proj(data, octree, depth - self.num_stages)


class Downsample(torch.nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: List[int] = (2,), nempty: bool = True,
                 conv_operands: str = "fp32"):
        super().__init__()
        self.norm = torch.nn.BatchNorm1d(out_channels)
        self.conv = OctreeConv(in_channels, out_channels, kernel_size, stride=2, nempty=nempty, use_bias=True)
        _set_conv_operands(self, conv_operands)

    def forward(self, data: torch.Tensor, octree, depth: int):
        return self.norm(self.conv(data, octree, depth))


class OctFormer(torch.nn.Module):
    """OctFormer-v1m1 (octformer_v1m1_base.py:495-615).  forward(data_dict) takes `coord`, `normal`, `feat`, `offset` and returns
    (n_points, num_classes).  The octree is built here, not by ocnn: node coordinates are
    floor((coord / octree_scale_factor + 1) * 2^(octree_depth - 1)), one torch.unique gives the leaves and the point -> leaf
    inverse, a leaf's feature is the mean of `feat` over its points, and OctreeInterp("nearest") is the leaf's row of each
    point.  No full layers are built: the coarsest depth in use must lie above octree_full_depth.  `normal` takes no part (the
    reference's patch_embed reads octree.features alone).
    conv_operands ("fp32", "bf16" or "autocast"; not a reference argument) is octree_conv's `operands` for every convolution of
    patch_embed, downsamples and decoder; the stem layers (Cin <= 8) keep their fp32 kernel."""

    def __init__(self, in_channels, num_classes, fpn_channels=168, channels=(96, 192, 384, 384), num_blocks=(2, 2, 18, 2),
                 num_heads=(6, 12, 24, 24), patch_size=26, stem_down=2, head_up=2, dilation=4, drop_path=0.5, nempty=True,
                 octree_scale_factor=10.24, octree_depth=11, octree_full_depth=2, conv_operands="fp32"):
        super().__init__()
        _nempty(nempty)
        self.patch_size = patch_size
        self.dilation = dilation
        self.nempty = nempty
        self.num_stages = len(num_blocks)
        self.stem_down = stem_down
        self.octree_scale_factor = octree_scale_factor
        self.octree_depth = octree_depth
        self.octree_full_depth = octree_full_depth
        if not octree_depth - stem_down - self.num_stages + 1 > octree_full_depth:
            raise ValueError("ao_amd octformer: depth %d - stem_down %d - %d stages + 1 must lie above octree_full_depth %d (no full "
                             "layers are built)" % (octree_depth, stem_down, self.num_stages, octree_full_depth))
        if head_up != stem_down:
            raise ValueError("ao_amd octformer: head_up %d != stem_down %d: the decoder must end at the leaves" % (head_up, stem_down))
        drop_ratio = torch.linspace(0, drop_path, sum(num_blocks)).tolist()

        self.patch_embed = PatchEmbed(in_channels, channels[0], stem_down, nempty, conv_operands=conv_operands)
        self.layers = torch.nn.ModuleList([
            OctFormerStage(dim=channels[i], num_heads=num_heads[i], patch_size=patch_size,
                           drop_path=drop_ratio[sum(num_blocks[:i]): sum(num_blocks[: i + 1])], dilation=dilation, nempty=nempty,
                           num_blocks=num_blocks[i])
            for i in range(self.num_stages)])
        self.downsamples = torch.nn.ModuleList([Downsample(channels[i], channels[i + 1], kernel_size=[2], nempty=nempty,
                                                           conv_operands=conv_operands)
                                                for i in range(self.num_stages - 1)])
        self.decoder = OctFormerDecoder(channels=channels, fpn_channel=fpn_channels, nempty=nempty, head_up=head_up,
                                        conv_operands=conv_operands)
        self.seg_head = (torch.nn.Sequential(torch.nn.Linear(fpn_channels, fpn_channels), torch.nn.BatchNorm1d(fpn_channels),
                                             torch.nn.ReLU(inplace=True), torch.nn.Linear(fpn_channels, num_classes))
                         if num_classes > 0 else torch.nn.Identity())

    def points2octree(self, coord, offset):
        """(OctreePyramid, the leaf row of every point)"""
        counts = torch.diff(offset.long(), prepend=offset.new_zeros(1).long())
        batch = torch.repeat_interleave(torch.arange(len(offset), device=coord.device), counts)
        node = torch.floor((coord.detach() / self.octree_scale_factor + 1.0) * 2.0 ** (self.octree_depth - 1)).long()
        uniq, inverse = torch.unique(torch.cat([batch.unsqueeze(1), node], dim=1), dim=0, return_inverse=True)
        octree = octree_pyramid(uniq[:, 1:], uniq[:, 0], self.octree_depth, self.stem_down + self.num_stages)
        leaf = octree.levels[0]
        rank = torch.empty_like(leaf.order)
        rank[leaf.order] = torch.arange(leaf.n, device=coord.device)
        return octree, rank[inverse]

    def forward(self, data_dict):
        coord, feat, offset = data_dict["coord"], data_dict["feat"], data_dict["offset"]
        octree, leaf_of = self.points2octree(coord, offset)
        n_leaf = octree.levels[0].n
        count = torch.bincount(leaf_of, minlength=n_leaf).to(feat.dtype).unsqueeze(1)
        feat = feat.new_zeros((n_leaf, feat.shape[1])).index_add(0, leaf_of, feat) / count

        feat = self.patch_embed(feat, octree, octree.depth)
        depth = octree.depth - self.stem_down
        features = {}
        for i in range(self.num_stages):
            depth_i = depth - i
            feat = self.layers[i](feat, octree.level(depth_i))
            features[depth_i] = feat
            if i < self.num_stages - 1:
                feat = self.downsamples[i](feat, octree, depth_i)
        out = self.decoder(features, octree)
        return self.seg_head(out[leaf_of])
