"""Instance-segmentation validation (pointcept/engines/hooks/evaluator.py: InsSegEvaluator of the reference; DESIGN.md
section 15): the association of a scene's proposals with its ground-truth instances on the device, and the AP tables on the host.

`associate` reads the (P, M) proposal masks once, in place, with one HIP kernel (ao_amd/csrc/inseval.hip, C ABI
include/ptv2_inseval_hip.h): per proposal the histogram of its set points over the ground-truth instances, its size and its
overlap with the void points -- exact integers.  The origin mapping of the reference (`pred_masks[:, idx]`) is folded into that
read as `nn_idx`.  What comes back is a `SceneMatches` record of small numpy arrays, never a list of dicts; `evaluate_matches`
restates the reference's greedy matching and AP integration over such records, in float64 on the host.

AO_AMD_INSEVAL=torch (read on every call) gives the same record from eager torch on the device: the A/B path.
"""
import os
from typing import NamedTuple

import numpy as np
import torch

from .. import _abi, _lib

BINS = _abi.inseval_consts["INSEVAL_BINS"]
MAX_PROPOSALS = _abi.inseval_consts["INSEVAL_MAX_PROPOSALS"]


class SceneMatches(NamedTuple):
    """One scene.  The G ground-truth instances in np.unique order of their ids, the Q kept proposals in row order; proposal q
    and instance g match when pred_class[q] == gt_segment_id[g] and inter[q, g] > 0."""
    gt_instance_id: np.ndarray   # (G) int64
    gt_segment_id: np.ndarray    # (G) int64
    gt_vert_count: np.ndarray    # (G) int64: all points carrying the id, whatever their segment
    pred_row: np.ndarray         # (Q) int64: row of pred_masks
    pred_class: np.ndarray       # (Q) int64
    pred_conf: np.ndarray        # (Q) float64: the fp32 score, widened
    pred_vert_count: np.ndarray  # (Q) int64
    pred_void: np.ndarray        # (Q) int64: set points whose segment is ignored
    inter: np.ndarray            # (Q, G) int64


def use_hip():
    mode = os.environ.get("AO_AMD_INSEVAL", "hip")
    if mode not in ("hip", "torch"):
        raise ValueError("ao_amd pointgroup: AO_AMD_INSEVAL=%r (hip or torch)" % (mode,))
    return mode == "hip"


def _isin(t, values):
    out = torch.zeros_like(t, dtype=torch.bool)
    for v in values:
        out |= t == int(v)
    return out


def gt_table(segment, instance, segment_ignore_index, instance_ignore_index):
    """Device tensors (ids (G), segment ids (G), counts (G), col (N), void (N)) of np.unique(instance, return_index=True,
    return_counts=True): ascending ids, the segment of the first occurrence, the count of all points carrying the id; kept are
    the ids != instance_ignore_index whose first-occurrence segment is not ignored.  col: the kept instance of each point or
    -1; void: the point's own segment is ignored."""
    n = instance.numel()
    void = _isin(segment, segment_ignore_index)
    ids, inverse = torch.unique(instance, return_inverse=True)
    counts = torch.bincount(inverse, minlength=ids.numel())
    first = torch.full((ids.numel(),), n, dtype=torch.int64, device=instance.device)
    first.scatter_reduce_(0, inverse, torch.arange(n, device=instance.device), "amin")
    seg_first = segment[first]
    keep = (ids != int(instance_ignore_index)) & ~_isin(seg_first, segment_ignore_index)
    col_of_id = torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full_like(ids, -1))
    return ids[keep], seg_first[keep], counts[keep], col_of_id[inverse], void


def _counts_hip(masks, nn_idx, col, void, g):
    """(inter (P, g), vert_count (P), void_inter (P)) int32 device tensors: one launch per window of BINS columns"""
    p, m = masks.shape
    n, dev = col.numel(), masks.device
    if p > MAX_PROPOSALS:
        raise ValueError("ao_amd pointgroup: %d proposals (at most %d)" % (p, MAX_PROPOSALS))
    vert = torch.zeros(p, dtype=torch.int32, device=dev)
    void_inter = torch.zeros(p, dtype=torch.int32, device=dev)
    if p == 0 or n == 0:  # empty tables, no launch
        return torch.zeros((p, g), dtype=torch.int32, device=dev), vert, void_inter
    L = _lib.lib()
    windows = []
    for g0 in range(0, max(g, 1), BINS):
        gw = min(BINS, g - g0)
        inside = (col >= g0) & (col < g0 + gw)
        code = (torch.where(inside, col - g0 + 1, torch.zeros_like(col)) * 2 + void.long()).int().contiguous()
        part = torch.empty((p, gw), dtype=torch.int32, device=dev)
        rc = L.inseval_associate_hip_launcher(p, m, n, gw, masks.data_ptr(), _lib.ptr(nn_idx), code.data_ptr(),
                                              part.data_ptr() if gw else None, vert.data_ptr(), void_inter.data_ptr(),
                                              _lib.stream_ptr())
        _lib.check(rc, "inseval_associate_hip_launcher")
        windows.append(part)
    return (windows[0] if len(windows) == 1 else torch.cat(windows, 1)), vert, void_inter


def _counts_torch(masks, nn_idx, col, void, g):
    """the same from eager torch: bincount of row * (g + 1) + col + 1 over the set elements"""
    p = masks.shape[0]
    is_set = masks != 0
    if nn_idx is not None:
        is_set = is_set[:, nn_idx.long()]
    rows, pts = is_set.nonzero(as_tuple=True)
    hist = torch.bincount(rows * (g + 1) + col[pts] + 1, minlength=p * (g + 1)).view(p, g + 1)
    return hist[:, 1:], is_set.sum(1), (is_set & void[None, :]).sum(1)


def associate(pred, segment, instance, num_classes, segment_ignore_index=(-1,), instance_ignore_index=-1, min_region_size=100,
              nn_idx=None):
    """InsSegEvaluator.associate_instances of the reference as a SceneMatches record.  pred: dict(pred_masks (P, M), pred_scores
    (P), pred_classes (P)); pred_masks a CUDA tensor (read in place) or a CPU tensor (uploaded once).  segment, instance (N)
    CUDA tensors; nn_idx (N) int32 or None (then N == M): point j reads column nn_idx[j] of the masks."""
    if not (segment.is_cuda and instance.is_cuda):
        raise RuntimeError("ao_amd.pointgroup.evaluate works on CUDA labels (no CPU fallback)")
    dev = segment.device
    segment, instance = segment.reshape(-1).long(), instance.reshape(-1).long()
    n = segment.numel()
    masks = pred["pred_masks"]
    classes = torch.as_tensor(pred["pred_classes"]).reshape(-1)
    scores = torch.as_tensor(pred["pred_scores"]).reshape(-1)
    if not (masks.dim() == 2 and classes.shape[0] == scores.shape[0] == masks.shape[0]):
        raise ValueError("ao_amd pointgroup: pred_masks %s, pred_scores %s, pred_classes %s" % (
            tuple(masks.shape), tuple(scores.shape), tuple(classes.shape)))
    if nn_idx is not None:
        _lib.require_cuda(nn_idx)
        nn_idx = nn_idx.reshape(-1).int().contiguous()
    if instance.numel() != n or (nn_idx.numel() if nn_idx is not None else masks.shape[1]) != n:
        raise ValueError("ao_amd pointgroup: %d segment labels, %d instance labels, masks of %d columns%s" % (
            n, instance.numel(), masks.shape[1], "" if nn_idx is None else ", %d nn_idx" % nn_idx.numel()))
    masks = masks.to(dev)  # (a CPU matrix is uploaded once; a device matrix is used in place)
    if masks.dtype != torch.int32:
        masks = (masks != 0).int()
    masks = masks.contiguous()
    hip = use_hip()

    ids, seg_ids, counts, col, void = gt_table(segment, instance, segment_ignore_index, instance_ignore_index)
    g = ids.numel()  # (a read-back: it sizes the table)
    inter, vert, void_inter = (_counts_hip if hip else _counts_torch)(masks, nn_idx, col, void, g)
    # one read-back for the six integer tables
    parts = [t.reshape(-1).long() for t in (ids, seg_ids, counts, vert, void_inter, inter)]
    packed = torch.cat(parts).cpu().numpy()
    ids, seg_ids, counts, vert, void_inter, inter = np.split(packed, np.cumsum([t.numel() for t in parts])[:-1])
    classes = classes.cpu().numpy().astype(np.int64)
    conf = scores.float().cpu().numpy().astype(np.float64)
    if num_classes is not None:
        valid = [i for i in range(int(num_classes)) if i not in segment_ignore_index]
        for what, have in (("ground-truth segment", seg_ids), ("predicted class", classes[~np.isin(classes, segment_ignore_index)])):
            if not np.isin(have, valid).all():
                raise ValueError("ao_amd pointgroup: a %s outside the %d classes: %s" % (what, num_classes, np.unique(have).tolist()))
    rows = np.nonzero(~np.isin(classes, segment_ignore_index) & (vert >= min_region_size))[0].astype(np.int64)
    return SceneMatches(ids, seg_ids, counts, rows, classes[rows], conf[rows], vert[rows], void_inter[rows],
                        inter.reshape(classes.shape[0], g)[rows])


def default_overlaps():
    return np.append(np.arange(0.5, 0.95, 0.05), 0.25)


def _average_precision(y_true, y_score, hard_false_negatives):
    """the reference's precision/recall build and integration (evaluator.py:425-477), statement for statement"""
    score_arg_sort = np.argsort(y_score)
    y_score_sorted = y_score[score_arg_sort]
    y_true_sorted = y_true[score_arg_sort]
    y_true_sorted_cumsum = np.cumsum(y_true_sorted)
    thresholds, unique_indices = np.unique(y_score_sorted, return_index=True)
    num_prec_recall = len(unique_indices) + 1
    num_examples = len(y_score_sorted)
    # (ScanNet pull request 26: every prediction unmatched and ignored leaves y_score empty)
    num_true_examples = y_true_sorted_cumsum[-1] if len(y_true_sorted_cumsum) > 0 else 0
    precision = np.zeros(num_prec_recall)
    recall = np.zeros(num_prec_recall)
    y_true_sorted_cumsum = np.append(y_true_sorted_cumsum, 0)  # (idx - 1 == -1 reads this 0)
    for idx_res, idx_scores in enumerate(unique_indices):
        cumsum = y_true_sorted_cumsum[idx_scores - 1]
        tp = num_true_examples - cumsum
        fp = num_examples - idx_scores - tp
        fn = cumsum + hard_false_negatives
        precision[idx_res] = float(tp) / (tp + fp)
        recall[idx_res] = float(tp) / (tp + fn)
    precision[-1] = 1.0  # the artificial last point
    recall[-1] = 0.0
    recall_for_conv = np.copy(recall)
    recall_for_conv = np.append(recall_for_conv[0], recall_for_conv)
    recall_for_conv = np.append(recall_for_conv, 0.0)
    step_widths = np.convolve(recall_for_conv, [-0.5, 0, 0.5], "valid")
    return np.dot(precision, step_widths)


def evaluate_matches(scenes, valid_class_ids, class_names, overlaps=None, min_region_size=100):
    """InsSegEvaluator.evaluate_matches of the reference over SceneMatches records: its `ap_scores` dict (all_ap, all_ap_50%,
    all_ap_25%, classes[name][ap | ap50% | ap25%]) plus "ap_table" (classes x overlaps).  The greedy state is reset per
    overlap; `overlap > th` is strict; ground truths below min_region_size leave the gt loop and count as ignored in an
    unmatched prediction; AP is 0.0 with gt and no prediction and NaN with no gt."""
    overlaps = default_overlaps() if overlaps is None else np.asarray(overlaps, dtype=np.float64)
    valid_class_ids, class_names = list(valid_class_ids), list(class_names)
    assert len(valid_class_ids) == len(class_names)
    ap_table = np.zeros((1, len(class_names), len(overlaps)), float)
    for oi, overlap_th in enumerate(overlaps):
        visited = [np.zeros(len(s.pred_row), dtype=bool) for s in scenes]
        for li, class_id in enumerate(valid_class_ids):
            y_true = np.empty(0)
            y_score = np.empty(0)
            hard_false_negatives = 0
            has_gt = False
            has_pred = False
            for s, seen in zip(scenes, visited):
                preds = np.nonzero(s.pred_class == class_id)[0]
                gts_all = np.nonzero(s.gt_segment_id == class_id)[0]
                gts = gts_all[s.gt_vert_count[gts_all] >= min_region_size]
                if len(gts):
                    has_gt = True
                if len(preds):
                    has_pred = True
                cur_true = np.ones(len(gts))
                cur_score = np.ones(len(gts)) * (-float("inf"))
                cur_match = np.zeros(len(gts), dtype=bool)
                for gti, g in enumerate(gts):
                    found_match = False
                    for q in preds[s.inter[preds, g] > 0]:
                        if seen[q]:
                            continue
                        inter = int(s.inter[q, g])
                        overlap = float(inter) / (int(s.gt_vert_count[g]) + int(s.pred_vert_count[q]) - inter)
                        if overlap > overlap_th:
                            confidence = s.pred_conf[q]
                            if cur_match[gti]:  # the lower score is a false positive; this prediction stays unvisited
                                max_score = max(cur_score[gti], confidence)
                                min_score = min(cur_score[gti], confidence)
                                cur_score[gti] = max_score
                                cur_true = np.append(cur_true, 0)
                                cur_score = np.append(cur_score, min_score)
                                cur_match = np.append(cur_match, True)
                            else:
                                found_match = True
                                cur_match[gti] = True
                                cur_score[gti] = confidence
                                seen[q] = True
                    if not found_match:
                        hard_false_negatives += 1
                cur_true = cur_true[cur_match]
                cur_score = cur_score[cur_match]
                for q in preds:
                    matched = gts_all[s.inter[q, gts_all] > 0]
                    inter = s.inter[q, matched].astype(np.float64)
                    overlap = inter / (s.gt_vert_count[matched] + s.pred_vert_count[q] - s.inter[q, matched])
                    if not (overlap > overlap_th).any():
                        small = s.gt_vert_count[matched] < min_region_size
                        num_ignore = int(s.pred_void[q]) + int(s.inter[q, matched][small].sum())
                        if float(num_ignore) / int(s.pred_vert_count[q]) <= overlap_th:
                            cur_true = np.append(cur_true, 0)
                            cur_score = np.append(cur_score, s.pred_conf[q])
                y_true = np.append(y_true, cur_true)
                y_score = np.append(y_score, cur_score)
            if has_gt and has_pred:
                ap_current = _average_precision(y_true, y_score, hard_false_negatives)
            elif has_gt:
                ap_current = 0.0
            else:
                ap_current = float("nan")
            ap_table[0, li, oi] = ap_current
    d_inf = 0
    o50 = np.where(np.isclose(overlaps, 0.5))
    o25 = np.where(np.isclose(overlaps, 0.25))
    o_all_but25 = np.where(np.logical_not(np.isclose(overlaps, 0.25)))
    ap_scores = dict()
    ap_scores["all_ap"] = np.nanmean(ap_table[d_inf, :, o_all_but25])
    ap_scores["all_ap_50%"] = np.nanmean(ap_table[d_inf, :, o50])
    ap_scores["all_ap_25%"] = np.nanmean(ap_table[d_inf, :, o25])
    ap_scores["classes"] = {}
    for li, label_name in enumerate(class_names):
        ap_scores["classes"][label_name] = {}
        ap_scores["classes"][label_name]["ap"] = np.average(ap_table[d_inf, li, o_all_but25])
        ap_scores["classes"][label_name]["ap50%"] = np.average(ap_table[d_inf, li, o50])
        ap_scores["classes"][label_name]["ap25%"] = np.average(ap_table[d_inf, li, o25])
    ap_scores["ap_table"] = ap_table[d_inf]
    return ap_scores


class InsSegEvaluator:
    """The reference's hook as a plain class: its constructor and attributes, `evaluate_scene` for one validation cloud,
    `evaluate` for a loader, `merge` for the per-rank lists."""

    def __init__(self, segment_ignore_index=(-1,), instance_ignore_index=-1):
        self.segment_ignore_index = segment_ignore_index
        self.instance_ignore_index = instance_ignore_index
        self.valid_class_names = None
        self.overlaps = default_overlaps()
        self.min_region_sizes = 100
        self.distance_threshes = float("inf")
        self.distance_confs = -float("inf")

    def evaluate_scene(self, model, input_dict, num_classes=None):
        """(loss, SceneMatches) of one cloud: one forward under no_grad, the proposals read on the device when the model has
        `propose_device`, the origin mapping (origin_coord / origin_segment / origin_instance) as nn_idx."""
        from .. import pointops

        assert len(input_dict["offset"]) == 1  # (the reference: one cloud per GPU)
        with torch.no_grad():
            if hasattr(model, "propose_device"):
                bias_pred, logit_pred = model.heads(model.backbone(input_dict))
                output_dict = model.losses(bias_pred, logit_pred, input_dict)
                scores, masks, classes = model.propose_device(input_dict["coord"], input_dict["offset"], bias_pred, logit_pred)
                output_dict.update(pred_scores=scores, pred_masks=masks, pred_classes=classes)
            else:
                output_dict = model(input_dict)
            segment, instance, nn_idx = input_dict["segment"], input_dict["instance"], None
            if "origin_coord" in input_dict.keys():
                nn_idx, _ = pointops.knn_query(1, input_dict["coord"].float(), input_dict["offset"].int(),
                                               input_dict["origin_coord"].float(), input_dict["origin_offset"].int())
                segment, instance = input_dict["origin_segment"], input_dict["origin_instance"]
            record = associate(output_dict, segment, instance, num_classes, self.segment_ignore_index,
                               self.instance_ignore_index, self.min_region_sizes, nn_idx)
        return float(output_dict["loss"]), record

    @staticmethod
    def merge(lists):
        """the per-rank lists of records as one list, rank after rank (the reference's flatten of comm.gather)"""
        return [scene for scenes in lists for scene in scenes]

    def evaluate(self, model, loader, names, num_classes, group=None):
        """The reference's eval(): `ap_scores` of the loader's scenes over all ranks, plus "loss" (this rank's mean)."""
        self.valid_class_names = [names[i] for i in range(num_classes) if i not in self.segment_ignore_index]
        valid_class_ids = [i for i in range(num_classes) if i not in self.segment_ignore_index]
        was_training = model.training
        model.eval()
        scenes, losses = [], []
        for input_dict in loader:
            input_dict = {k: v.cuda(non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in input_dict.items()}
            loss, record = self.evaluate_scene(model, input_dict, num_classes)
            scenes.append(record)
            losses.append(loss)
        model.train(was_training)
        lists = [scenes]
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            lists = [None] * dist.get_world_size(group)
            dist.all_gather_object(lists, scenes, group=group)
        ap_scores = evaluate_matches(self.merge(lists), valid_class_ids, self.valid_class_names, self.overlaps,
                                     self.min_region_sizes)
        ap_scores["loss"] = float(np.mean(losses)) if losses else float("nan")
        return ap_scores
