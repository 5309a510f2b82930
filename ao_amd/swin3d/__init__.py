"""Swin3D-v1m1's window attention blocks on HIP: everything inside the reference's BasicLayer except
`downsample`.  The stem, GridDownsample / GridKNNDownsample, Upsample and the whole-model registration follow MinkowskiEngine's
conventions and are a follow-up."""
from .model import BasicLayer, Mlp, SwinTransformerBlock, WindowAttention, crse_signals
from .ops import crse_attention, crse_attention_torch, crse_rows, window_pairs
from .window import WindowMap, window_map

__all__ = ["BasicLayer", "Mlp", "SwinTransformerBlock", "WindowAttention", "crse_signals", "crse_attention",
           "crse_attention_torch", "crse_rows", "window_pairs", "WindowMap", "window_map"]
