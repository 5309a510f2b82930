"""PointGroup (PG-v1m1, pointcept/models/point_group/point_group_v1m1_base.py) on the MI355X: the reference's constructor
keywords, state-dict keys (`backbone.*`, `bias_head.0/1/3.*`, `seg_head.*`) and returned dict, over ao_amd/pointgroup/ops.py.

Two deliberate differences from the reference: when no point survives `segment_ignore_index` the
reference indexes a 1-D tensor with [:, 0] and raises, this returns empty outputs with masks of shape (0, N); and the dense
(nCluster, N) matrix is never formed: only the kept proposals get a mask row.
"""
from functools import partial

import torch
import torch.nn as nn

from .. import _lib
from ..ptv2.segmentor import cross_entropy
from . import ops

DEFAULT_BACKBONE = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                        layers=(2, 3, 4, 6, 2, 2, 2, 2))


def _build_backbone(backbone):
    if isinstance(backbone, nn.Module):
        return backbone
    cfg = dict(DEFAULT_BACKBONE if backbone is None else backbone)
    kind = cfg.pop("type", "SpUNet-v1m1")
    if kind != "SpUNet-v1m1":
        raise ValueError("ao_amd pointgroup: backbone type %r (a config dict resolves to SpUNet-v1m1; pass any other backbone "
                         "as an nn.Module)" % (kind,))
    from ..spunet import SpUNetBase

    cfg["num_classes"] = 0  # (the headless form: the backbone returns its features)
    return SpUNetBase(**cfg)


class PointGroup(nn.Module):
    def __init__(self, backbone=None, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1,
                 segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300,
                 cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02):
        super().__init__()
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.semantic_num_classes = semantic_num_classes
        self.segment_ignore_index = segment_ignore_index
        self.semantic_ignore_index = semantic_ignore_index
        self.instance_ignore_index = instance_ignore_index
        self.cluster_thresh = cluster_thresh
        self.cluster_closed_points = cluster_closed_points
        self.cluster_propose_points = cluster_propose_points
        self.cluster_min_points = cluster_min_points
        self.voxel_size = voxel_size
        self.backbone = _build_backbone(backbone)
        self.bias_head = nn.Sequential(
            nn.Linear(backbone_out_channels, backbone_out_channels),
            norm_fn(backbone_out_channels),
            nn.ReLU(),
            nn.Linear(backbone_out_channels, 3),
        )
        self.seg_head = nn.Linear(backbone_out_channels, semantic_num_classes)

    def heads(self, feat):
        """(bias_pred (n, 3), logit_pred (n, classes)) of the backbone's features"""
        return self.bias_head(feat), self.seg_head(feat)

    def losses(self, bias_pred, logit_pred, data_dict):
        seg_loss = cross_entropy(logit_pred, data_dict["segment"], self.semantic_ignore_index)
        bias_l1_loss, bias_cosine_loss = ops.bias_loss(bias_pred, data_dict["coord"], data_dict["instance_center"],
                                                       data_dict["instance"], self.instance_ignore_index)
        loss = seg_loss + bias_l1_loss + bias_cosine_loss
        return dict(loss=loss, seg_loss=seg_loss, bias_l1_loss=bias_l1_loss, bias_cosine_loss=bias_cosine_loss)

    @torch.no_grad()
    def propose_device(self, coord, offset, bias_pred, logit_pred):
        """(pred_scores (P) fp32, pred_masks (P, N) int32, pred_classes (P) int64) on the device: the clusters of the shifted
        points (coord + bias_pred) / voxel_size within cluster_thresh among the points whose predicted class is not ignored.
        What ao_amd/pointgroup/evaluate.py reads in place: the masks never leave the device."""
        _lib.require_cuda(coord, offset, bias_pred, logit_pred)
        n = coord.shape[0]
        center_pred = ((coord.float() + bias_pred.float()) / self.voxel_size)
        prob = torch.softmax(logit_pred.float(), dim=-1)
        segment_pred = torch.max(prob, 1)[1]
        mask = torch.ones_like(segment_pred, dtype=torch.bool)
        for index in self.segment_ignore_index:
            mask &= segment_pred != index
        kept = mask.nonzero().view(-1)
        if kept.numel() == 0:  # (the reference raises here)
            dev = coord.device
            return (torch.zeros(0, device=dev), torch.zeros((0, n), dtype=torch.int32, device=dev),
                    torch.zeros(0, dtype=torch.int64, device=dev))
        offset = offset.long()
        batch = torch.searchsorted(offset, kept, right=True)  # offset2batch(offset)[mask]
        counts = torch.bincount(batch, minlength=offset.numel())
        offset_ = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
        label = segment_pred[kept].int()
        idx, start_len, capped = ops.ball_query(center_pred[kept].contiguous(), offset_, self.cluster_thresh)
        sub_cluster, sizes, firsts = ops.cluster(label, idx, start_len, self.cluster_min_points, capped)
        point_cluster = torch.full((n,), -1, dtype=torch.int32, device=coord.device)
        point_cluster[kept] = sub_cluster
        scores, masks, classes = ops.proposals(point_cluster, sizes, kept[firsts.long()].int(), segment_pred, prob,
                                               self.cluster_propose_points)
        return scores, masks, classes

    @torch.no_grad()
    def propose(self, coord, offset, bias_pred, logit_pred):
        """propose_device(...) as CPU tensors: what the reference's forward returns"""
        scores, masks, classes = self.propose_device(coord, offset, bias_pred, logit_pred)
        return scores.cpu(), masks.cpu(), classes.cpu()

    def forward(self, data_dict):
        feat = self.backbone(data_dict)
        bias_pred, logit_pred = self.heads(feat)
        return_dict = self.losses(bias_pred, logit_pred, data_dict)
        if not self.training:
            scores, masks, classes = self.propose(data_dict["coord"], data_dict["offset"], bias_pred, logit_pred)
            return_dict["pred_scores"] = scores
            return_dict["pred_masks"] = masks
            return_dict["pred_classes"] = classes
        return return_dict
