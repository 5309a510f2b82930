"""Stratified Transformer (ST-v1m2) on HIP: pair lists, the pointops2 attention operators, the fused window attention, the
KPConv stem and the model (ao_amd/csrc/stratified.hip, kpconv.hip, include/ptv2_st_hip.h)."""
from .ops import (PairSet, attention_step1_v2, attention_step2_with_rel_pos_value_v2, build_pairs, cells,  # noqa: F401
                  dot_prod_with_idx_v3, quant_grid_length, rel_index, scatter_softmax_csr, transpose_csr, window_attention)
from .kpconv import FastBatchNorm1d, KPConvLayer, ball_query, kernel_points, weighted_features  # noqa: F401
from .model import StratifiedTransformer  # noqa: F401
