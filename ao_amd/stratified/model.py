"""Stratified Transformer (ST-v1m2, pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py) on the MI355X:
the reference's constructor keywords and defaults, returned logits and state-dict keys and shapes, over ao_amd/stratified/ops.py
and kpconv.py.  fp32 only; under autocast the attention and KPConv nodes take fp32 inputs.

What differs from the reference: a BasicLayer builds its two pair sets (plain and shifted windows, each by query and by key) once
and its blocks reuse them, where the reference rebuilds masks, gathers, a sort and a bincount in every block; the attention of a
block is one autograd node (ops.window_attention); `data_dict` may carry a precomputed `neighbor_idx`.
"""
import torch
import torch.nn as nn

from . import ops
from .kpconv import FastBatchNorm1d, KPConvLayer, ball_query


def _p2():
    from ..pointops2 import pointops  # (at call time: pointops2.pointops itself imports this package's operators)

    return pointops


def new_offset_truncated(offset, ratio):
    """BasicLayer.forward :340-346: every cloud's share is truncated before it is added"""
    ends, out, count, prev = [int(v) for v in offset.tolist()], [], 0, 0
    for e in ends:
        count += int((e - prev) * ratio) + 1
        out.append(count)
        prev = e
    return out


def new_offset_accumulated(offset, ratio):
    """TransitionDown.forward :449-455: the first entry is truncated, the later ones accumulate a float that torch.IntTensor
    truncates when the list becomes a tensor -- from the third cloud on this can differ from new_offset_truncated"""
    ends = [int(v) for v in offset.tolist()]
    out = [int(ends[0] * ratio) + 1]
    count = int(ends[0] * ratio) + 1
    for i in range(1, len(ends)):
        count += ((ends[i] - ends[i - 1]) * ratio) + 1
        out.append(int(count))  # (IntTensor truncates towards zero; the sum is positive)
    return out


class DropPath(nn.Module):
    """stochastic depth per sample (timm.models.layers.DropPath)"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * mask.div_(keep)


class WindowAttention(nn.Module):
    def __init__(self, embed_channels, num_heads, window_size, quant_size, attn_drop=0.0, proj_drop=0.0, scale=None,
                 rel_query=True, rel_key=True, rel_value=True, qkv_bias=True):
        super().__init__()
        if not (rel_query and rel_key and rel_value):
            raise NotImplementedError("ao_amd stratified: ST-v1m2 with rel_query = rel_key = rel_value = True only (the configs' flags)")
        if attn_drop:
            raise NotImplementedError("ao_amd stratified: attn_drop is not provided (the reference constructs it and never applies it)")
        self.embed_channels = embed_channels
        self.head_channels = embed_channels // num_heads
        self.num_heads = num_heads
        self.scale = scale or self.head_channels ** -0.5
        self.window_size = window_size
        self.quant_size = quant_size
        self.quant_grid_length = ops.quant_grid_length(window_size, quant_size)
        shape = (2 * self.quant_grid_length, self.num_heads, self.head_channels, 3)
        self.relative_pos_query_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_key_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_value_table = nn.Parameter(torch.zeros(shape))
        for _ in range(3):  # (:101, :109, :117 all initialise the QUERY table; the other two start at zero)
            nn.init.trunc_normal_(self.relative_pos_query_table, std=0.02)
        self.qkv = nn.Linear(embed_channels, embed_channels * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop, inplace=True)
        self.proj = nn.Linear(embed_channels, embed_channels)
        self.proj_drop = nn.Dropout(proj_drop, inplace=True)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, feats, coords, pairs):
        n, c = feats.shape
        qkv = self.qkv(feats).reshape(n, 3, self.num_heads, c // self.num_heads).permute(1, 0, 2, 3).contiguous()
        query, key, value = qkv[0], qkv[1], qkv[2]
        query = query * self.scale
        x = ops.window_attention(query, key, value, coords, pairs, self.relative_pos_query_table, self.relative_pos_key_table,
                                 self.relative_pos_value_table, self.window_size, self.quant_size)
        x = self.proj(x.to(feats.dtype))
        return self.proj_drop(x)


class MLP(nn.Module):
    def __init__(self, in_channels, hidden_channels=None, out_channels=None, drop=0.0):
        super().__init__()
        out_channels = out_channels or in_channels
        hidden_channels = hidden_channels or in_channels
        self.fc1 = nn.Linear(in_channels, hidden_channels)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_channels, out_channels)
        self.drop = nn.Dropout(drop, inplace=True)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class Block(nn.Module):
    def __init__(self, embed_channels, num_heads, window_size, quant_size, mlp_expend_ratio=4.0, drop_path=0.0, qk_scale=None,
                 rel_query=True, rel_key=True, rel_value=True, qkv_bias=True):
        super().__init__()
        self.norm1 = nn.LayerNorm(embed_channels)
        self.attn = WindowAttention(embed_channels, num_heads, window_size, quant_size, scale=qk_scale, rel_query=rel_query,
                                    rel_key=rel_key, rel_value=rel_value, qkv_bias=qkv_bias)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = nn.LayerNorm(embed_channels)
        self.mlp = MLP(in_channels=embed_channels, hidden_channels=int(embed_channels * mlp_expend_ratio))

    def forward(self, feats, coords, pairs):
        short_cut = feats
        feats = self.attn(self.norm1(feats), coords, pairs)
        feats = short_cut + self.drop_path(feats)
        return feats + self.drop_path(self.mlp(self.norm2(feats)))


class TransitionDown(nn.Module):
    def __init__(self, in_channels, out_channels, ratio, k, norm_layer=nn.LayerNorm):
        super().__init__()
        self.ratio = ratio
        self.k = k
        self.norm = norm_layer(in_channels) if norm_layer else None
        self.linear = nn.Linear(in_channels, out_channels, bias=False)
        self.pool = nn.MaxPool1d(k)

    def forward(self, feats, coords, offset):
        P = _p2()
        new_offset = torch.tensor(new_offset_accumulated(offset, self.ratio), dtype=torch.int32, device=offset.device)
        idx = P.furthestsampling(coords, offset, new_offset)
        new_coords = coords[idx.long(), :]
        feats = P.queryandgroup(self.k, coords, new_coords, feats.contiguous(), None, offset, new_offset, use_xyz=False)
        m, k, c = feats.shape
        feats = self.linear(self.norm(feats.view(m * k, c)).view(m, k, c)).transpose(1, 2).contiguous()
        return self.pool(feats).squeeze(-1), new_coords, new_offset


class TransitionUp(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.linear1 = nn.Sequential(nn.LayerNorm(out_channels), nn.Linear(out_channels, out_channels))
        self.linear2 = nn.Sequential(nn.LayerNorm(in_channels), nn.Linear(in_channels, out_channels))

    def forward(self, feats, coords, offset, skip_feats, skip_coords, skip_offset):
        feats = self.linear1(skip_feats) + _p2().interpolation(coords, skip_coords, self.linear2(feats).contiguous(), offset, skip_offset)
        return feats, skip_coords, skip_offset


class BasicLayer(nn.Module):
    def __init__(self, embed_channels, out_channels, depth, num_heads, window_size, quant_size, mlp_expend_ratio=4.0,
                 down_ratio=0.25, down_num_sample=16, drop_path=None, qk_scale=None, down=True, rel_query=True, rel_key=True,
                 rel_value=True, qkv_bias=True):
        super().__init__()
        self.depth = depth
        self.window_size = window_size
        self.quant_size = quant_size
        self.down_ratio = down_ratio
        if isinstance(drop_path, list):
            assert len(drop_path) == depth
        elif isinstance(drop_path, float):
            drop_path = [drop_path for _ in range(depth)]
        else:
            drop_path = [0.0 for _ in range(depth)]
        self.blocks = nn.ModuleList([
            Block(embed_channels, num_heads, window_size, quant_size, mlp_expend_ratio=mlp_expend_ratio, drop_path=drop_path[i],
                  qk_scale=qk_scale, rel_query=rel_query, rel_key=rel_key, rel_value=rel_value, qkv_bias=qkv_bias)
            for i in range(depth)])
        self.down = TransitionDown(embed_channels, out_channels, down_ratio, down_num_sample) if down else None

    def forward(self, feats, coords, offset):
        # the sampled points of the large windows: one farthest-point sampling per level (:340-348)
        new_offset = torch.tensor(new_offset_truncated(offset, self.down_ratio), dtype=torch.int32, device=offset.device)
        down_idx = _p2().furthestsampling(coords, offset.int(), new_offset)
        # the two pair sets of the level, each by query and by key; block i takes the plain windows for even i (:368-372)
        pairs = [ops.build_pairs(coords, offset, down_idx, self.window_size, shifted) for shifted in (False, True)[:min(self.depth, 2)]]
        for i, blk in enumerate(self.blocks):
            feats = blk(feats, coords, pairs[i % 2])
        if self.down:
            feats_down, coords_down, offset_down = self.down(feats, coords, offset)
        else:
            feats_down, coords_down, offset_down = None, None, None
        return feats, coords, offset, feats_down, coords_down, offset_down


class KPConvSimpleBlock(nn.Module):
    def __init__(self, in_channels, out_channels, prev_grid_size, sigma=1.0, negative_slope=0.2, bn_momentum=0.02):
        super().__init__()
        self.kpconv = KPConvLayer(in_channels, out_channels, point_influence=prev_grid_size * sigma, add_one=False)
        self.bn = FastBatchNorm1d(out_channels, momentum=bn_momentum)
        self.activation = nn.LeakyReLU(negative_slope=negative_slope)

    def forward(self, feats, xyz, batch, neighbor_idx):
        return self.activation(self.bn(self.kpconv(xyz, xyz, neighbor_idx, feats)))


class KPConvResBlock(nn.Module):
    def __init__(self, in_channels, out_channels, prev_grid_size, sigma=1.0, negative_slope=0.2, bn_momentum=0.02):
        super().__init__()
        d_2 = out_channels // 4
        activation = nn.LeakyReLU(negative_slope=negative_slope)
        self.unary_1 = nn.Sequential(nn.Linear(in_channels, d_2, bias=False), FastBatchNorm1d(d_2, momentum=bn_momentum), activation)
        self.unary_2 = nn.Sequential(nn.Linear(d_2, out_channels, bias=False), FastBatchNorm1d(out_channels, momentum=bn_momentum),
                                     activation)
        self.kpconv = KPConvLayer(d_2, d_2, point_influence=prev_grid_size * sigma, add_one=False)
        self.bn = FastBatchNorm1d(out_channels, momentum=bn_momentum)   # (constructed and never applied, as in the reference)
        self.activation = activation
        if in_channels != out_channels:
            self.shortcut_op = nn.Sequential(nn.Linear(in_channels, out_channels, bias=False),
                                             FastBatchNorm1d(out_channels, momentum=bn_momentum))
        else:
            self.shortcut_op = nn.Identity()

    def forward(self, feats, xyz, batch, neighbor_idx):
        shortcut = feats
        feats = self.unary_1(feats)
        feats = self.kpconv(xyz, xyz, neighbor_idx, feats)
        feats = self.unary_2(feats)
        return feats + self.shortcut_op(shortcut)


class StratifiedTransformer(nn.Module):
    def __init__(self, in_channels, num_classes, channels=(48, 96, 192, 384, 384), num_heads=(6, 12, 24, 24), depths=(3, 9, 3, 3),
                 window_size=(0.2, 0.4, 0.8, 1.6), quant_size=(0.01, 0.02, 0.04, 0.08), mlp_expend_ratio=4.0, down_ratio=0.25,
                 down_num_sample=16, kp_ball_radius=2.5 * 0.02, kp_max_neighbor=34, kp_grid_size=0.02, kp_sigma=1.0,
                 drop_path_rate=0.2, rel_query=True, rel_key=True, rel_value=True, qkv_bias=True, stem=True):
        super().__init__()
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.kp_ball_radius = kp_ball_radius
        self.kp_max_neighbor = kp_max_neighbor
        self.stem = stem
        if stem:
            self.point_embed = nn.ModuleList([KPConvSimpleBlock(in_channels, channels[0], kp_grid_size, sigma=kp_sigma),
                                              KPConvResBlock(channels[0], channels[0], kp_grid_size, sigma=kp_sigma)])
            self.down = TransitionDown(channels[0], channels[1], down_ratio, down_num_sample)
        else:
            assert channels[0] == channels[1]
            self.point_embed = nn.ModuleList([KPConvSimpleBlock(in_channels, channels[1], kp_grid_size, sigma=kp_sigma)])
        num_layers = len(depths)
        self.layers = nn.ModuleList([
            BasicLayer(embed_channels=channels[i + 1], out_channels=channels[i + 2] if i < num_layers - 1 else channels[i + 1],
                       depth=depths[i], num_heads=num_heads[i], window_size=window_size[i], quant_size=quant_size[i],
                       mlp_expend_ratio=mlp_expend_ratio, down_ratio=down_ratio, down_num_sample=down_num_sample,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], rel_query=rel_query, rel_key=rel_key, rel_value=rel_value,
                       qkv_bias=qkv_bias, down=i < num_layers - 1)
            for i in range(num_layers)])
        self.up = nn.ModuleList([TransitionUp(channels[i + 1], channels[i]) for i in reversed(range(1, num_layers))])
        if self.stem:
            self.up.append(TransitionUp(channels[1], channels[0]))
        self.classifier = nn.Sequential(nn.Linear(channels[0], channels[0]), nn.BatchNorm1d(channels[0]), nn.ReLU(inplace=True),
                                        nn.Linear(channels[0], num_classes))
        self.init_weights()

    def forward(self, data_dict):
        feats = data_dict["feat"].float()
        coords = data_dict["coord"].float().contiguous()
        offset = data_dict["offset"].int()
        neighbor_idx = data_dict.get("neighbor_idx")
        if neighbor_idx is None:
            neighbor_idx = ball_query(self.kp_ball_radius, self.kp_max_neighbor, coords, offset)
        feats_stack, coords_stack, offset_stack = [], [], []
        for layer in self.point_embed:
            feats = layer(feats, coords, None, neighbor_idx)
        feats = feats.contiguous()
        if self.stem:
            feats_stack.append(feats)
            coords_stack.append(coords)
            offset_stack.append(offset)
            feats, coords, offset = self.down(feats, coords, offset)
        for layer in self.layers:
            feats, coords, offset, feats_down, coords_down, offset_down = layer(feats, coords, offset)
            feats_stack.append(feats)
            coords_stack.append(coords)
            offset_stack.append(offset)
            feats, coords, offset = feats_down, coords_down, offset_down
        feats, coords, offset = feats_stack.pop(), coords_stack.pop(), offset_stack.pop()
        for up in self.up:
            feats, coords, offset = up(feats, coords, offset, feats_stack.pop(), coords_stack.pop(), offset_stack.pop())
        return self.classifier(feats)

    def init_weights(self):
        def _init_weights(m):
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.LayerNorm, nn.BatchNorm1d)):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

        self.apply(_init_weights)
