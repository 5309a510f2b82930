"""`from pointops2 import pointops` / `import pointops2.pointops` compatible module."""
import torch

from ..pointops.aggregation import aggregation  # noqa: F401
from ..pointops.grouping import grouping2 as grouping  # noqa: F401  (pointops2 `grouping` is the CUDA op, :58-89)
from ..pointops.interpolation import interpolation_index_weight, _InterpolateRows
from ..pointops.query import knn_query_dist2
from ..pointops.sampling import farthest_point_sampling as furthestsampling  # noqa: F401
from ..pointops.subtraction import subtraction  # noqa: F401
from ..stratified.ops import (attention_step1_v2, attention_step2_with_rel_pos_value_v2,  # noqa: F401  (:169-257, :853-960,
                              dot_prod_with_idx_v3)                                        # :631-754)


def knnquery(nsample, xyz, new_xyz, offset, new_offset):
    """pointops2 argument order (:36-55); placeholder index is the segment start (knnquery_cuda_kernel.cu:90)."""
    if new_xyz is None:
        new_xyz, new_offset = xyz, offset
    idx, dist2 = knn_query_dist2(nsample, xyz, offset, new_xyz, new_offset, pad_with_start=True)
    return idx, torch.sqrt(dist2)


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True, return_indx=False):
    """:963-1001 -- plain gather (no -1 masking), relative xyz prepended."""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    if new_xyz is None:
        new_xyz = xyz
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    grouped_feat = grouping(feat, idx)
    out = grouped_feat
    if use_xyz:
        grouped_xyz = grouping(xyz, idx) - new_xyz.unsqueeze(1)
        out = torch.cat((grouped_xyz, grouped_feat), -1)
    return (out, idx) if return_indx else out


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """:1112-1127"""
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    idx, weight = interpolation_index_weight(xyz, new_xyz, offset, new_offset, k)
    return _InterpolateRows.apply(feat, idx, weight)


interpolation2 = interpolation


def _not_provided(name):
    def op(*args, **kwargs):
        raise NotImplementedError("pointops2.%s is not provided: ST-v1m2 with rel_query = rel_key = rel_value = True calls "
                                  "attention_step1_v2, dot_prod_with_idx_v3 and attention_step2_with_rel_pos_value_v2 only" % name)
    op.__name__ = name
    return op


# the older forms of the three operators above; no ST-v1m2 code path with the configs' flags reaches them
attention_step1 = _not_provided("attention_step1")
attention_step2 = _not_provided("attention_step2")
attention_step2_v2 = _not_provided("attention_step2_v2")
dot_prod_with_idx = _not_provided("dot_prod_with_idx")
dot_prod_with_idx_v2 = _not_provided("dot_prod_with_idx_v2")
attention_step2_with_rel_pos_value = _not_provided("attention_step2_with_rel_pos_value")
