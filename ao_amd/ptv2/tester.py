"""Whole-scene test-time inference: the reference's SemSegTester (pointcept/engines/test.py:33-234), the number every
`configs/*/semseg-pt-v2m2-*.py` ends in (`test = dict(type="SemSegTester")`).

A scene is cut into fragments (one GridSample(mode="test") fragment list per test-time augmentation, ao_amd/ptv2/transform.py::
test_fragments or the reference's own dataset), the network runs on every fragment, `softmax(logits)` is added into a per-point
vote table and the prediction is the table's argmax (test.py:94-123).

The vote runs on ao_amd/csrc/vote.hip: one launch pair per fragment that reads each logit once and updates the table in
place (the reference: a softmax, a gather, an add and a scatter per fragment with two (n, C) temporaries, and a python loop
over `offset` that reads every bound back from the device).  Contract: a fragment holds a point at most once, which
GridSample(mode="test") and SphereCrop(mode="all") guarantee; the segments of a collated batch are issued one after the
other in list order, so the table is bitwise what adding the fragments one at a time gives.  CPU tensors and
AO_AMD_VOTE=torch take an eager formulation with the same per-segment order (the A/B path, as AO_AMD_LOVASZ=torch).

A row index outside the table: the HIP path writes nothing for that segment and for every later one, records it in a device
word, and `VoteTable.raise_if_invalid()` (one synchronisation; SemSegTester calls it once per scene, `add(check=True)` at the
call) raises.  The eager path indexes as torch does.
"""
import logging
import os
import time

import numpy as np
import torch

from . import evaluate
from .transform import point_collate


def _use_hip(t):
    return t.is_cuda and os.environ.get("AO_AMD_VOTE", "hip") != "torch"


class VoteTable:
    """(n_points, num_classes) fp32 sums of per-fragment softmax outputs: `votes`; `add` one fragment or a collated batch of
    fragments; `predict()` the first maximal class per point, (n_points,) int64 on the table's device."""

    def __init__(self, n_points, num_classes, device):
        self.n_points, self.num_classes = int(n_points), int(num_classes)
        self.votes = torch.zeros((self.n_points, self.num_classes), dtype=torch.float32, device=device)
        self._status = torch.zeros(1, dtype=torch.int32, device=device) if self.votes.is_cuda else None

    def _bounds(self, n, offset, offset_host):
        if offset is None and offset_host is None:
            return [n]
        if offset_host is None:
            offset_host = offset.tolist()  # ONE read-back; a batch made by point_collate carries offset_host
        return [int(e) for e in offset_host]

    def add(self, seg_logits, index, offset=None, check=False, offset_host=None):
        """votes[index[s:e]] += softmax(seg_logits[s:e]) for every segment (s, e) of `offset` (None: one segment), in order.
        seg_logits (n, C) fp32 or bf16; index (n,) int64 or int32, no duplicates inside a segment.  check=True validates
        the contract (a sort and a synchronisation per call): for tests."""
        if seg_logits.dim() != 2 or seg_logits.shape[1] != self.num_classes or index.shape != seg_logits.shape[:1]:
            raise ValueError("VoteTable.add: logits %s, index %s, table %s"
                             % (tuple(seg_logits.shape), tuple(index.shape), tuple(self.votes.shape)))
        bounds = self._bounds(seg_logits.shape[0], offset, offset_host)
        if not bounds or bounds[-1] != seg_logits.shape[0] or any(b < a for a, b in zip([0] + bounds[:-1], bounds)):
            raise ValueError("VoteTable.add: offset %s does not partition %d rows" % (bounds, seg_logits.shape[0]))
        if check:
            start = 0
            for end in bounds:
                part = index[start:end].long()
                if part.numel() and (int(part.min()) < 0 or int(part.max()) >= self.n_points):
                    raise IndexError("VoteTable.add: an index of rows %d:%d is outside [0, %d)" % (start, end, self.n_points))
                if part.numel() and bool((torch.sort(part)[0].diff() == 0).any()):
                    raise ValueError("VoteTable.add: rows %d:%d name a point twice (a fragment holds a point at most once)"
                                     % (start, end))
                start = end
        if _use_hip(self.votes):
            self._add_hip(seg_logits, index, bounds)
        else:
            start = 0
            for end in bounds:  # test.py:110-113
                self.votes[index[start:end].long(), :] += torch.softmax(seg_logits[start:end].float(), -1)
                start = end
        return self

    def _add_hip(self, seg_logits, index, bounds):
        from .. import _lib

        _lib.require_cuda(seg_logits, index)
        if seg_logits.dtype not in (torch.float32, torch.bfloat16):
            seg_logits = seg_logits.float()
        if index.dtype not in (torch.int64, torch.int32):
            index = index.long()
        seg_logits, index = seg_logits.contiguous(), index.contiguous()
        L, c, st = _lib.lib(), self.num_classes, _lib.stream_ptr()
        bf16, i64 = int(seg_logits.dtype == torch.bfloat16), int(index.dtype == torch.int64)
        lp, ip = seg_logits.data_ptr(), index.data_ptr()
        lrow, irow = c * seg_logits.element_size(), index.element_size()
        start = 0
        for end in bounds:
            rc = L.seg_vote_add_hip_launcher(end - start, c, lp + start * lrow, bf16, ip + start * irow, i64,
                                             self.votes.data_ptr(), self.n_points, self._status.data_ptr(), st)
            _lib.check(rc, "seg_vote_add_hip_launcher")
            start = end

    def raise_if_invalid(self):
        """One synchronisation: raises when an `add` since the last call met a row outside the table (HIP path)."""
        if self._status is not None and _use_hip(self.votes):
            from .. import _lib

            if _lib.lib().seg_vote_status_hip_launcher(self._status.data_ptr(), _lib.stream_ptr()) != 0:
                raise IndexError("VoteTable: a fragment named a point outside [0, %d); that fragment and every later one "
                                 "were not added" % self.n_points)

    def predict(self):
        if not _use_hip(self.votes):
            return self.votes.max(1)[1]
        from .. import _lib

        pred = torch.empty(self.n_points, dtype=torch.int64, device=self.votes.device)
        rc = _lib.lib().seg_vote_argmax_hip_launcher(self.n_points, self.num_classes, self.votes.data_ptr(), pred.data_ptr(),
                                                     _lib.stream_ptr())
        _lib.check(rc, "seg_vote_argmax_hip_launcher")
        return pred


def _model_device(model):
    p = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
    return p.device if p is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")


def test_scene(model, fragment_list, n_points, num_classes, fragment_batch=1, autocast=None, device=None, table=None,
               empty_cache=False, on_batch=None):
    """The fragment loop of test.py:94-123 for one scene: the VoteTable after every fragment went through `model`.
    fragment_batch fragments are collated into one forward (the reference: 1).  In eval mode every op of the network is
    segment-local and BatchNorm uses its running statistics, so batching changes rounding only.  autocast: a dtype for
    torch.autocast around the forward (None: off).  No host synchronisation per fragment beyond what `model` itself does."""
    device = _model_device(model) if device is None else torch.device(device)
    table = VoteTable(n_points, num_classes, device) if table is None else table
    fragment_batch = max(int(fragment_batch), 1)
    for s_i in range(0, len(fragment_list), fragment_batch):
        input_dict = point_collate(fragment_list[s_i:s_i + fragment_batch])
        for key in input_dict.keys():
            if isinstance(input_dict[key], torch.Tensor):
                input_dict[key] = input_dict[key].to(device, non_blocking=True)
        with torch.no_grad():
            if autocast is not None:
                with torch.autocast(device_type=device.type, dtype=autocast):
                    seg_logits = model(input_dict)["seg_logits"]
            else:
                seg_logits = model(input_dict)["seg_logits"]
        if empty_cache and device.type == "cuda":
            torch.cuda.empty_cache()
        table.add(seg_logits, input_dict["index"], input_dict["offset"], offset_host=input_dict.get("offset_host"))
        if on_batch is not None:
            on_batch(s_i, min(s_i + fragment_batch, len(fragment_list)))
    return table


test_scene.__test__ = False  # (a library function, not a pytest case, whatever module imports it)


def _counts_numpy(pred, segment, k, ignore_index):
    """intersection_and_union of pointcept/utils/misc.py:40-55 as the (3, k) int64 table of evaluate.confusion_counts"""
    pred, segment = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(segment).reshape(-1).astype(np.int64)
    keep = segment != ignore_index
    pred, segment = pred[keep], segment[keep]
    inside = (pred >= 0) & (pred < k)
    hit = pred[inside & (pred == segment)]
    tgt = segment[(segment >= 0) & (segment < k)]
    return np.stack([np.bincount(hit, minlength=k), np.bincount(pred[inside], minlength=k), np.bincount(tgt, minlength=k)])


class SemSegTester:
    """test.py:33-234.  `tester(cfg, test_loader, model)` runs every scene of the loader, writes `<cfg.save_path>/result/
    test_epoch<cfg.test_epoch>/<name>_pred.npy` (an existing file is loaded instead: the reference's resume), for
    cfg.dataset_type == "ScanNetDataset" also `submit/<name>.txt`, logs the reference's lines to the "pointcept" logger and
    returns evaluate.summarize() of the totals over all ranks.  fragment_batch: fragments per forward (the reference: 1;
    DESIGN.md section 3.8d gives the measured reason for the default); autocast: dtype or None."""

    UNSUPPORTED = ("SemanticKITTIDataset", "NuScenesDataset")

    def __init__(self, fragment_batch=8, autocast=None):
        self.fragment_batch, self.autocast = fragment_batch, autocast

    @staticmethod
    def collate_fn(batch):
        return batch

    def __call__(self, cfg, test_loader, model):
        assert test_loader.batch_size == 1
        if cfg.dataset_type in self.UNSUPPORTED:
            raise NotImplementedError("SemSegTester: the submission formats of SemanticKITTIDataset and NuScenesDataset "
                                      "are not on this path (got %s)" % cfg.dataset_type)
        logger = logging.getLogger("pointcept")
        logger.info(">>>>>>>>>>>>>>>> Start Evaluation >>>>>>>>>>>>>>>>")
        dist = torch.distributed
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        main = not multi or dist.get_rank() == 0
        k, ignore = int(cfg.data.num_classes), int(cfg.data.ignore_index)
        device = _model_device(model)
        model.eval()
        save_path = os.path.join(cfg.save_path, "result", "test_epoch{}".format(cfg.test_epoch))
        os.makedirs(save_path, exist_ok=True)
        if cfg.dataset_type == "ScanNetDataset" and main:
            os.makedirs(os.path.join(save_path, "submit"), exist_ok=True)
        if multi:
            dist.barrier()
        total = np.zeros((3, k), dtype=np.int64)
        spent, scenes = 0.0, 0
        for idx, data_dict in enumerate(test_loader):
            end = time.time()
            data_dict = dict(data_dict[0])  # batch size 1
            fragment_list = data_dict.pop("fragment_list")
            segment = data_dict.pop("segment")
            data_name = data_dict.pop("name")
            n_points = int(segment.shape[0])
            pred_save_path = os.path.join(save_path, "{}_pred.npy".format(data_name))
            if os.path.isfile(pred_save_path):
                logger.info("{}/{}: {}, loaded pred and label.".format(idx + 1, len(test_loader), data_name))
                pred = np.load(pred_save_path)
                seg_host = segment.cpu().numpy() if torch.is_tensor(segment) else np.asarray(segment)
                counts = _counts_numpy(pred, seg_host, k, ignore)
            else:
                def log_batch(s_i, e_i, _idx=idx, _name=data_name, _num=len(fragment_list)):
                    logger.info("Test: {}/{}-{}, Batch: {}/{}".format(_idx + 1, len(test_loader), _name, s_i, _num))

                table = test_scene(model, fragment_list, n_points, k, self.fragment_batch, self.autocast, device=device,
                                   empty_cache=bool(getattr(cfg, "empty_cache", False)), on_batch=log_batch)
                pred_dev = table.predict()
                if pred_dev.is_cuda:
                    counts = evaluate.confusion_counts(pred_dev, torch.as_tensor(segment).to(device), k, ignore).cpu().numpy()
                pred = pred_dev.cpu().numpy()
                table.raise_if_invalid()
                if not pred_dev.is_cuda:
                    counts = _counts_numpy(pred, torch.as_tensor(segment).numpy(), k, ignore)
                np.save(pred_save_path, pred)
            intersection, target = counts[0].astype(np.float64), counts[2].astype(np.float64)
            union = (counts[1] + counts[2] - counts[0]).astype(np.float64)
            total += counts
            # test.py:132-138
            mask = union != 0
            iou_class = intersection / (union + 1e-10)
            iou = np.mean(iou_class[mask])
            acc = sum(intersection) / (sum(target) + 1e-10)
            t_i, t_t = total[0].astype(np.float64), total[2].astype(np.float64)
            t_u = (total[1] + total[2] - total[0]).astype(np.float64)
            m_iou = np.mean(t_i / (t_u + 1e-10))
            m_acc = np.mean(t_i / (t_t + 1e-10))
            spent, scenes = spent + time.time() - end, scenes + 1
            logger.info("Test: {} [{}/{}]-{} Batch {:.3f} ({:.3f}) Accuracy {:.4f} ({:.4f}) mIoU {:.4f} ({:.4f})".format(
                data_name, idx + 1, len(test_loader), n_points, time.time() - end, spent / scenes, acc, m_acc, iou, m_iou))
            if cfg.dataset_type == "ScanNetDataset":
                np.savetxt(os.path.join(save_path, "submit", "{}.txt".format(data_name)),
                           np.asarray(test_loader.dataset.class2id)[pred].reshape([-1, 1]), fmt="%d")
        logger.info("Syncing ...")
        if multi:  # the sums the reference takes over its gathered meters (test.py:199-208)
            t = torch.from_numpy(total).to(device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t)
            total = t.cpu().numpy()
        result = evaluate.summarize(total[0], total[1] + total[2] - total[0], total[2])
        if main:
            logger.info("Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}".format(result["mIoU"], result["mAcc"], result["allAcc"]))
            for i in range(k):
                logger.info("Class_{idx} - {name} Result: iou/accuracy {iou:.4f}/{accuracy:.4f}".format(
                    idx=i, name=cfg.data.names[i], iou=result["iou_class"][i], accuracy=result["acc_class"][i]))
            logger.info("<<<<<<<<<<<<<<<<< End Evaluation <<<<<<<<<<<<<<<<<")
        return result
