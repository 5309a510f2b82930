"""Masked Scene Contrast (MSC-v1m1, pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py) on the MI355X:
the reference's constructor keywords and defaults, state-dict keys (`backbone.*`, `mask_token`, `color_head.*`, `normal_head.*`)
and returned dict, over ao_amd/msc/ops.py.  MaskedSceneContrastCSC is MSC-v1m2 (masked_scene_contrast_v1m2_csc.py): the same
forward with the partitioned InfoNCE loss of ops.csc_nce, which reads the unaugmented coordinates and the unmixed offsets
(DESIGN.md section 16).

What differs from the reference: the (M, M) similarity matrix and the padded patch-to-point map are never
formed; no matched pair raises ValueError where the reference returns a NaN loss; nothing is read back in the loss; with more than one rank the returned nce_loss
is the local loss plus the other ranks' detached losses, divided by the world size -- the reference's value, with the gradient
the reference's all-reduce (which cuts the graph) does not have; and mixing two scenes that share a voxel raises ValueError,
because the sparse-convolution tables hold one row per voxel.
"""
import random

import torch
import torch.distributed as dist
import torch.nn as nn

from ..pointgroup.model import _build_backbone
from . import ops


def _world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _mixed_offset(offset):
    """:250-252: every two scenes become one cloud"""
    return torch.cat([offset[1:-1:2], offset[-1].unsqueeze(0)], dim=0)


class MaskedSceneContrast(nn.Module):
    def __init__(self, backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0,
                 view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4,
                 contrast_weight=1, reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True):
        super().__init__()
        self.backbone = _build_backbone(backbone)
        self.mask_grid_size = mask_grid_size
        self.mask_rate = mask_rate
        self.view1_mix_prob = view1_mix_prob
        self.view2_mix_prob = view2_mix_prob
        self.matching_max_k = matching_max_k
        self.matching_max_radius = matching_max_radius
        self.matching_max_pair = matching_max_pair
        self.nce_t = nce_t
        self.contrast_weight = contrast_weight
        self.reconstruct_weight = reconstruct_weight
        self.reconstruct_color = reconstruct_color
        self.reconstruct_normal = reconstruct_normal

        self.mask_token = nn.Parameter(torch.zeros(1, backbone_in_channels))
        torch.nn.init.trunc_normal_(self.mask_token, mean=0.0, std=0.02)
        self.color_head = nn.Linear(backbone_out_channels, 3) if reconstruct_color else None
        self.normal_head = nn.Linear(backbone_out_channels, 3) if reconstruct_normal else None

    def generate_cross_masks(self, view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, perm=None, generator=None):
        return ops.cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, self.mask_grid_size,
                               self.mask_rate, perm=perm, generator=generator)

    def match_contrastive_pair(self, view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius, row_draws=None,
                               perm=None, generator=None):
        return ops.match_pairs(view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius, self.matching_max_pair,
                               row_draws=row_draws, perm=perm, generator=generator)

    def compute_contrastive_loss(self, view1_feat, view1_offset, view2_feat, view2_offset, match_index):
        assert view1_offset.shape == view2_offset.shape
        return self._over_ranks(*ops.info_nce(view1_feat, view2_feat, match_index, self.nce_t))

    @staticmethod
    def _over_ranks(loss, pos_sim, neg_sim):
        world = _world_size()
        if world > 1:
            # :195-203.  The reference all-reduces the loss itself, which cuts its graph; here the sum over the ranks is taken
            # of a detached copy and the local loss keeps its place in it, so the value is the reference's and the gradient
            # is that of the local loss / world
            total = loss.detach().clone()
            dist.all_reduce(total)
            loss = loss + (total - loss.detach())
            pos_sim, neg_sim = pos_sim.clone(), neg_sim.clone()
            dist.all_reduce(pos_sim)
            dist.all_reduce(neg_sim)
        return loss / world, pos_sim / world, neg_sim / world

    def _contrastive_loss(self, view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord, view2_offset,
                          match_index):
        return self.compute_contrastive_loss(view1_feat, view1_offset, view2_feat, view2_offset, match_index)

    def _backbone(self, data, which, mixed):
        try:
            return self.backbone(data)
        except ValueError as e:
            if mixed and "same voxel" in str(e):
                raise ValueError("ao_amd msc: view %d was mixed (view%d_mix_prob = %r) and two of its merged scenes put a row on "
                                 "the same voxel; the sparse-convolution tables hold one row per voxel (DESIGN.md section 13)"
                                 % (which, which, getattr(self, "view%d_mix_prob" % which))) from e
            raise

    def forward(self, data_dict, mix=None, draws=None):
        """mix: (bool, bool), whether view 1 / view 2 is mixed; None tosses random.random() against view*_mix_prob as the
        reference does.  draws: an optional dict of the random tensors, for replay: mask_perm, row_draws, pair_perm (see
        ops.cross_masks and ops.match_pairs), and generator, a torch.Generator for those not given."""
        draws = draws or {}
        view1_origin_coord = data_dict["view1_origin_coord"]
        view1_coord = data_dict["view1_coord"]
        view1_feat = data_dict["view1_feat"]
        view1_offset = data_dict["view1_offset"].int()

        view2_origin_coord = data_dict["view2_origin_coord"]
        view2_coord = data_dict["view2_coord"]
        view2_feat = data_dict["view2_feat"]
        view2_offset = data_dict["view2_offset"].int()

        # the masks come from the unaugmented coordinates of both views together
        view1_point_mask, view2_point_mask = self.generate_cross_masks(
            view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, perm=draws.get("mask_perm"),
            generator=draws.get("generator"))

        view1_mask_tokens = self.mask_token.expand(view1_coord.shape[0], -1)
        view1_weight = view1_point_mask.unsqueeze(-1).type_as(view1_mask_tokens)
        view1_feat = view1_feat * (1 - view1_weight) + view1_mask_tokens * view1_weight

        view2_mask_tokens = self.mask_token.expand(view2_coord.shape[0], -1)
        view2_weight = view2_point_mask.unsqueeze(-1).type_as(view2_mask_tokens)
        view2_feat = view2_feat * (1 - view2_weight) + view2_mask_tokens * view2_weight

        view1_data_dict = dict(origin_coord=view1_origin_coord, coord=view1_coord, feat=view1_feat, offset=view1_offset)
        view2_data_dict = dict(origin_coord=view2_origin_coord, coord=view2_coord, feat=view2_feat, offset=view2_offset)

        # (a sparse-convolution backbone reads the voxel coordinates)
        if "view1_discrete_coord" in data_dict.keys():
            view1_data_dict["discrete_coord"] = data_dict["view1_discrete_coord"]
        if "view2_discrete_coord" in data_dict.keys():
            view2_data_dict["discrete_coord"] = data_dict["view2_discrete_coord"]

        # view mixing: every two scenes of a view become one cloud
        if mix is None:
            mix = (random.random() < self.view1_mix_prob, random.random() < self.view2_mix_prob)
        if mix[0]:
            view1_data_dict["offset"] = _mixed_offset(view1_offset)
        if mix[1]:
            view2_data_dict["offset"] = _mixed_offset(view2_offset)

        view1_feat = self._backbone(view1_data_dict, 1, mix[0])
        view2_feat = self._backbone(view2_data_dict, 2, mix[1])
        match_index = self.match_contrastive_pair(
            view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, max_k=self.matching_max_k,
            max_radius=self.matching_max_radius, row_draws=draws.get("row_draws"), perm=draws.get("pair_perm"),
            generator=draws.get("generator"))
        nce_loss, pos_sim, neg_sim = self._contrastive_loss(view1_feat, view1_origin_coord, view1_offset, view2_feat,
                                                            view2_origin_coord, view2_offset, match_index)
        loss = nce_loss * self.contrast_weight
        result_dict = dict(nce_loss=nce_loss, pos_sim=pos_sim, neg_sim=neg_sim)

        if self.color_head is not None:
            assert "view1_color" in data_dict.keys()
            assert "view2_color" in data_dict.keys()
            view1_color = data_dict["view1_color"]
            view2_color = data_dict["view2_color"]
            view1_color_pred = self.color_head(view1_feat[view1_point_mask])
            view2_color_pred = self.color_head(view2_feat[view2_point_mask])
            color_loss = (
                torch.sum((view1_color_pred - view1_color[view1_point_mask]) ** 2)
                + torch.sum((view2_color_pred - view2_color[view2_point_mask]) ** 2)
            ) / (view1_color_pred.shape[0] + view2_color_pred.shape[0])
            loss = loss + color_loss * self.reconstruct_weight
            result_dict["color_loss"] = color_loss

        if self.normal_head is not None:
            assert "view1_normal" in data_dict.keys()
            assert "view2_normal" in data_dict.keys()
            view1_normal = data_dict["view1_normal"]
            view2_normal = data_dict["view2_normal"]
            view1_normal_pred = self.normal_head(view1_feat[view1_point_mask])
            view2_normal_pred = self.normal_head(view2_feat[view2_point_mask])

            view1_normal_pred = view1_normal_pred / (torch.norm(view1_normal_pred, p=2, dim=1, keepdim=True) + 1e-10)
            view2_normal_pred = view2_normal_pred / (torch.norm(view2_normal_pred, p=2, dim=1, keepdim=True) + 1e-10)
            # (the reference's sign: a plain sum of dot products)
            normal_loss = (
                torch.sum(view1_normal_pred * view1_normal[view1_point_mask])
                + torch.sum(view2_normal_pred * view2_normal[view2_point_mask])
            ) / (view1_normal_pred.shape[0] + view2_normal_pred.shape[0])
            loss = loss + normal_loss * self.reconstruct_weight
            result_dict["normal_loss"] = normal_loss

        result_dict["loss"] = loss
        return result_dict


class MaskedSceneContrastCSC(MaskedSceneContrast):
    """MSC-v1m2: the reference's keywords and defaults (r2 = 2 there; its ScanNet config sets r1 = 2, r2 = 20, mask_rate = 0 and
    no heads), the state-dict keys of MSC-v1m1, and the same returned dict."""

    def __init__(self, backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0,
                 view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4,
                 contrast_weight=1, reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True, partitions=4, r1=0.125,
                 r2=2):
        super().__init__(backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=mask_grid_size, mask_rate=mask_rate,
                         view1_mix_prob=view1_mix_prob, view2_mix_prob=view2_mix_prob, matching_max_k=matching_max_k,
                         matching_max_radius=matching_max_radius, matching_max_pair=matching_max_pair, nce_t=nce_t,
                         contrast_weight=contrast_weight, reconstruct_weight=reconstruct_weight,
                         reconstruct_color=reconstruct_color, reconstruct_normal=reconstruct_normal)
        self.partitions = partitions
        self.r1 = r1
        self.r2 = r2

    def compute_partitions(self, coord1, coord2):
        """:182-200, the eager statements: (len(coord2), len(coord1)) fp32 with -1e7, 0, 1, 2, 3.  The loss does not form it."""
        return ops.compute_partitions_torch(coord1, coord2, self.r1, self.r2)

    def compute_contrastive_loss(self, view1_feat, view1_coord, view1_offset, view2_feat, view2_coord, view2_offset, match_index):
        assert view1_offset.shape == view2_offset.shape
        return self._over_ranks(*ops.csc_nce(view1_feat, view2_feat, view1_coord, view2_coord, view1_offset, match_index,
                                             self.nce_t, self.r1, self.r2, self.partitions))

    def _contrastive_loss(self, view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord, view2_offset,
                          match_index):
        return self.compute_contrastive_loss(view1_feat, view1_origin_coord, view1_offset, view2_feat, view2_origin_coord,
                                             view2_offset, match_index)
