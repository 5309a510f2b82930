"""Point Transformer V1 (PointTransformer-Seg26 / 38 / 50) on the MI355X: ao_amd/ptv1/model.py, with the vector-attention layer
on ao_amd/csrc/ptv1.hip (ao_amd/ptv1/attention.py)."""
from .attention import attention_torch, vector_attention
from .model import (Bottleneck, LayerNorm1d, PointTransformerLayer, PointTransformerSeg, PointTransformerSeg26,
                    PointTransformerSeg38, PointTransformerSeg50, TransitionDown, TransitionUp)

__all__ = ["attention_torch", "vector_attention", "Bottleneck", "LayerNorm1d", "PointTransformerLayer", "PointTransformerSeg",
           "PointTransformerSeg26", "PointTransformerSeg38", "PointTransformerSeg50", "TransitionDown", "TransitionUp"]
