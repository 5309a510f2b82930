"""Masked Scene Contrast (MSC-v1m1): self-supervised pretraining of the sparse U-Net on the MI355X."""
from . import ops
from .model import MaskedSceneContrast
from .ops import cross_masks, info_nce, info_nce_torch, match_pairs, patch_ids

__all__ = ["MaskedSceneContrast", "cross_masks", "info_nce", "info_nce_torch", "match_pairs", "ops", "patch_ids"]
