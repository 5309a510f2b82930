"""Masked Scene Contrast (MSC-v1m1, and MSC-v1m2 with the CSC partitions): self-supervised pretraining of the sparse U-Net on
the MI355X (DESIGN.md sections 13 and 16)."""
from . import ops
from .model import MaskedSceneContrast, MaskedSceneContrastCSC
from .ops import cross_masks, csc_nce, csc_nce_torch, info_nce, info_nce_torch, match_pairs, patch_ids

__all__ = ["MaskedSceneContrast", "MaskedSceneContrastCSC", "cross_masks", "csc_nce", "csc_nce_torch", "info_nce", "info_nce_torch",
           "match_pairs", "ops", "patch_ids"]
