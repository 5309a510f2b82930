"""PointGroup (PG-v1m1) instance segmentation on the MI355X: ao_amd/pointgroup/model.py over the operators of
ao_amd/pointgroup/ops.py on ao_amd/csrc/pointgroup.hip (C ABI include/ptv2_pg_hip.h), and its validation,
ao_amd/pointgroup/evaluate.py on ao_amd/csrc/inseval.hip (C ABI include/ptv2_inseval_hip.h)."""
from .evaluate import InsSegEvaluator, SceneMatches, associate, evaluate_matches
from .model import PointGroup
from .ops import (BALL_CAP, ball_query, ballquery_batch_p, bfs_cluster, bias_loss, bias_loss_torch, cluster, proposals)

__all__ = ["PointGroup", "InsSegEvaluator", "SceneMatches", "associate", "evaluate_matches", "BALL_CAP", "ball_query", "ballquery_batch_p", "bfs_cluster", "bias_loss", "bias_loss_torch", "cluster",
           "proposals"]
