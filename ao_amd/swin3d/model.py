"""Swin3D's attention blocks of one stage (pointcept/models/swin3d/swin3d_layers.py:383-876 of the reference) with the
reference's constructor arguments and state-dict keys, on the operators of ops.py.

BasicLayer.forward(feats, grid_coord, batch, local_xyz, colors) replaces the reference's (sp, coords_sp) pair of MinkowskiEngine
tensors: `feats` (n, C); `grid_coord` (n, 3) integer voxel coordinates at the level's own stride 1; `batch` (n); `local_xyz`
(n, 3) the sub-voxel offset of the point, in voxels; `colors` (n, 3 or 6) colour and normal in [-1, 1].  It returns the features.
LayerNorm, the Linears, GELU and the residuals stay torch.  `fp16_mode` is handed to crse_attention: with 1 ("fp16 forward and
fp32 backward") or 2 the attention runs on half-precision storage wherever the qkv Linear wrote float16, i.e. under fp16 autocast
(DESIGN.md section 22); 2 ("fp16 both ways") takes the same path as 1, a half-precision backward is not built.  With 0, or
outside autocast, the attention is fp32.
"""
import torch
from torch import nn

from ..stratified.model import DropPath
from .ops import crse_attention
from .window import window_map

MODES = ("XYZ", "XYZ_RGB", "XYZ_RGB_NORM")


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def crse_signals(wmap, local_xyz, colors, quant_size, cRSE):
    """(n, 3 S) fp32 in the sorted order of `wmap`: get_index01's n_coords (:801-805) times the quant sizes of
    WindowAttention.forward (:515-537): (w_w_xyz + local_xyz) quant_size, then colour and normal times 2 quant_size."""
    order = wmap.order.long()
    parts = [(wmap.w_w_xyz.float() + local_xyz.float()[order]) * quant_size]
    if "RGB" in cRSE:
        parts.append(colors.float()[order, 0:3] * (2 * quant_size))
    if "NORM" in cRSE:
        parts.append(colors.float()[order, 3:6] * (2 * quant_size))
    return torch.cat(parts, dim=1).contiguous()


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, quant_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0,
                 cRSE="XYZ_RGB", fp16_mode=0):
        super().__init__()
        if attn_drop or proj_drop:
            raise NotImplementedError("ao_amd swin3d: attn_drop / proj_drop other than 0 (the reference never sets them)")
        if cRSE not in MODES:
            raise ValueError("ao_amd swin3d: cRSE %r; one of %s" % (cRSE, ", ".join(MODES)))
        self.dim, self.window_size, self.num_heads, self.quant_size = dim, window_size, num_heads, quant_size
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.color_windowsize = self.normal_windowsize = 2   # colour and normal lie in [-1, 1]
        self.fp16_mode, self.cRSE = fp16_mode, cRSE
        self.table_rows = []
        for key, rows in (("xyz", window_size * quant_size), ("rgb", 2 * (2 * quant_size)), ("norm", 2 * (2 * quant_size))):
            if key.upper() not in cRSE:
                continue
            self.table_rows.append(rows)
            for role in ("query", "key", "value"):
                table = nn.Parameter(torch.zeros(3, 2 * rows, num_heads, head_dim))
                nn.init.trunc_normal_(table, std=0.02)
                setattr(self, "%s_%s_table" % (role, key), table)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def tables(self, role):
        return torch.cat([getattr(self, "%s_%s_table" % (role, key)).view(-1) for key in ("xyz", "rgb", "norm") if key.upper() in self.cRSE])

    def forward(self, feats, attn_args):
        wmap, signals = attn_args
        out = crse_attention(self.qkv(feats), wmap, signals, self.tables("query"), self.tables("key"), self.tables("value"),
                             self.table_rows, self.scale, self.num_heads, fp16_mode=self.fp16_mode)
        return self.proj(out)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, quant_size, drop_path=0.0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, cRSE="XYZ_RGB", fp16_mode=0):
        super().__init__()
        self.window_size = window_size
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=window_size, quant_size=quant_size, num_heads=num_heads, qkv_bias=qkv_bias,
                                    qk_scale=qk_scale, cRSE=cRSE, fp16_mode=fp16_mode)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)

    def forward(self, feats, attn_args):
        feats = feats + self.drop_path(self.attn(self.norm1(feats), attn_args))
        return feats + self.drop_path(self.mlp(self.norm2(feats)))


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, quant_size, out_channels=None, mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, down_stride=2, cRSE="XYZ_RGB", fp16_mode=0):
        super().__init__()
        if downsample is not None:
            raise NotImplementedError("ao_amd swin3d: BasicLayer(downsample=...): GridDownsample and GridKNNDownsample follow "
                                      "MinkowskiEngine's pooling conventions and are the follow-up (DESIGN.md section 21)")
        self.window_size, self.depth, self.dim, self.num_heads = window_size, depth, dim, num_heads
        self.quant_size, self.cRSE, self.fp16_mode = quant_size, cRSE, fp16_mode
        self.shift_size = window_size // 2
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim, num_heads, window_size, quant_size,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, mlp_ratio=mlp_ratio,
                                 qkv_bias=qkv_bias, qk_scale=qk_scale, norm_layer=norm_layer, cRSE=cRSE, fp16_mode=fp16_mode)
            for i in range(depth)])
        self.downsample = None

    def attn_args(self, grid_coord, batch, local_xyz, colors, shift):
        wmap = window_map(grid_coord, batch, self.window_size, shift)
        return wmap, crse_signals(wmap, local_xyz, colors, self.quant_size, self.cRSE)

    def forward(self, feats, grid_coord, batch, local_xyz, colors):
        plain = self.attn_args(grid_coord, batch, local_xyz, colors, 0)
        shifted = self.attn_args(grid_coord, batch, local_xyz, colors, self.shift_size) if self.depth > 1 else None
        for i, blk in enumerate(self.blocks):
            feats = blk(feats, plain if i % 2 == 0 else shifted)
        return feats

    def extra_repr(self) -> str:
        return "window_size=%d, depth=%d, channel=%d, num_heads=%d, quant_size=%d, cRSE=%s, fp16_mode=%d" % (
            self.window_size, self.depth, self.dim, self.num_heads, self.quant_size, self.cRSE, self.fp16_mode)
