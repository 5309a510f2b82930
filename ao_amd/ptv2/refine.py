"""REAL's epoch-end label refinement on the device: prompts from the basket's logits, votes from the predictor's masks.

Reference (pointcept/engines/train_sam_real.py, once per whole scene at the end of every epoch):

    :333-338  seg_pred = argmax(logits), -1 where the basket never saw the row; confidence = softmax top-two margin
    :353-391  on a 0.5 m x / y grid, one prompt per (cell, class present in the scene): the most confident point whose
              pseudo-label disagrees with the prediction, if its confidence is above 0.9
    :397-474  per view: the prompts visible in it go to SAM; every mask whose confident points' most frequent prediction is
              the prompt's class votes for that class on all of its points
    :488-512  where the vote's argmax agrees with the prediction the pseudo-label is rewritten

The reference does this in numpy with a python loop over cells x classes (a full-n boolean mask each) and fancy indexing
per mask.  Here each stage is a launch of ao_amd/csrc/refine.hip (C ABI: include/ptv2_refine_hip.h).  The mask predictor is
NOT part of this module: `masks_for` is the caller's (SAM in the reference).  The reference's quirks are kept as they are
(DESIGN.md section 8): the two differently parenthesised cell counts, strict cell boundaries, `mask[u - 1][v - 1]` with
numpy's wrap of index -1, the cleared `mask[0, 0]`.

Host synchronisations: `begin` reads the prompt count once (and, when no `bounds` are passed, the x / y extent once);
`vote_view` reads which prompts the view sees (the predictor is host-driven anyway); `finish(check=False)` reads nothing.

There is no CPU fallback.  AO_AMD_REFINE=torch runs the same contract in eager torch on the device (the A/B path, as
AO_AMD_VOTE=torch).
"""
import math
import os

import numpy as np
import torch

from .. import _abi, _lib

_K = _abi.refine_consts
MIN_C, MAX_C = _K["PTV2_REFINE_MIN_C"], _K["PTV2_REFINE_MAX_C"]
_ERROR, _PROMPTS, _UPDATED = (_K["PTV2_REFINE_STATUS_" + n] for n in ("ERROR", "PROMPTS", "UPDATED"))
_BAD_PIXEL, _BAD_CLASS, _BAD_CAPACITY = (_K["PTV2_REFINE_BAD_" + n] for n in ("PIXEL", "CLASS", "CAPACITY"))
UNSEEN = -100.0  # what the basket fills a row with that no step wrote (basket.py)


def _use_hip():
    return os.environ.get("AO_AMD_REFINE", "hip") != "torch"


def _classes(c):
    c = int(c)
    if not MIN_C <= c <= MAX_C:
        raise ValueError("ao_amd refine: %d classes, supported are %d..%d" % (c, MIN_C, MAX_C))
    return c


def _new_status(device):
    return torch.zeros(_K["PTV2_REFINE_STATUS_WORDS"], dtype=torch.int32, device=device)


def _raise_for(error):
    if error & _BAD_PIXEL:
        raise IndexError("ao_amd refine: a visible point's pixel (u, v) lies outside [0, height] x [0, width]; it was skipped")
    if error & _BAD_CLASS:
        raise IndexError("ao_amd refine: a prediction or prompt class outside the class range; it was skipped")
    if error & _BAD_CAPACITY:
        raise RuntimeError("ao_amd refine: more prompts than the output arrays hold")


def _first_argmax(t):
    """first maximal column of every row, as np.argmax (torch.argmax does not promise which of equal maxima it returns)"""
    cols = torch.arange(t.shape[1], device=t.device).expand_as(t)
    return torch.where(t == t.max(1, keepdim=True).values, cols, t.shape[1]).min(1).values


def grid_cells(lo_x, hi_x, lo_y, hi_y, grid=0.5):
    """(nx, ny) of train_sam_real.py:362,366, parenthesised as there: nx = int(ceil(Lx) // grid), ny = int(ceil(Ly // grid)),
    the lengths in float32.  The y strip beyond ny * grid belongs to no cell; the x cells run past the extent."""
    lx = np.float32(hi_x) - np.float32(lo_x)
    ly = np.float32(hi_y) - np.float32(lo_y)
    if not (np.isfinite(lx) and np.isfinite(ly)):
        raise ValueError("ao_amd refine: the x / y extent is not finite")
    nx = int(math.ceil(lx) // grid)
    ny = int(math.ceil(np.floor_divide(ly, np.float32(grid))))
    return max(nx, 0), max(ny, 0)


def scene_confidence(logits):
    """logits (n, C) fp32 -> pred (n,) int32: first maximal class, -1 for a row the basket never saw (logits[i, 0] == -100);
    conf (n,) fp32: top-two margin of the fp32 softmax."""
    _lib.require_cuda(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("ao_amd refine: logits must be (n, C) float32, got %s %s" % (tuple(logits.shape), logits.dtype))
    n, c = logits.shape[0], _classes(logits.shape[1])
    logits = logits.contiguous()
    if not _use_hip():
        pred = _first_argmax(logits).int()
        pred = torch.where(logits[:, 0] == UNSEEN, torch.full_like(pred, -1), pred)
        top = torch.softmax(logits, 1).topk(2, dim=1).values
        return pred, top[:, 0] - top[:, 1]
    pred = torch.empty(n, dtype=torch.int32, device=logits.device)
    conf = torch.empty(n, dtype=torch.float32, device=logits.device)
    rc = _lib.lib().refine_confidence_hip_launcher(n, c, logits.data_ptr(), pred.data_ptr(), conf.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "refine_confidence_hip_launcher")
    return pred, conf


def _xy_bounds(coord):
    """(lo_x, hi_x, lo_y, hi_y) of a device coord: the exact bounds launcher of the augmentation, one read"""
    from .transform import aug_bounds

    b = aug_bounds(coord)[:6].tolist()
    return b[0], b[3], b[1], b[4]


def _prompts_torch(coord, pred, conf, label, present, lo_x, lo_y, nx, ny, grid, threshold, status):
    n, c, dev = coord.shape[0], present.shape[0], coord.device

    def cell(x, lo, cells):
        steps = (torch.arange(cells + 1, dtype=torch.float64, device=dev) * grid).float()
        bound = torch.tensor(lo, dtype=torch.float32, device=dev) + steps
        j = torch.searchsorted(bound, x.contiguous())  # bound[j - 1] < x <= bound[j]
        ok = (j >= 1) & (j <= cells) & (x < bound[j.clamp(max=cells)])
        return j - 1, ok

    ix, okx = cell(coord[:, 0], lo_x, nx)
    iy, oky = cell(coord[:, 1], lo_y, ny)
    k = pred.long()
    cand = okx & oky & (k >= 0) & (k < c) & (conf > threshold) & (label.long() != k)
    cand &= present.bool()[k.clamp(0, c - 1)]
    rows = torch.nonzero(cand).reshape(-1)
    key = (ix[rows] * ny + iy[rows]) * c + k[rows]
    best = torch.full((nx * ny * c,), -1.0, dtype=torch.float32, device=dev).scatter_reduce(0, key, conf[rows], "amax")
    rows, key = rows[conf[rows] == best[key]], key[conf[rows] == best[key]]
    winner = torch.full((nx * ny * c,), n, dtype=torch.int64, device=dev).scatter_reduce(0, key, rows, "amin")
    slots = torch.nonzero(winner < n).reshape(-1)  # ascending == (ix, iy, class) order
    status[_PROMPTS] = slots.numel()
    return winner[slots].int(), (slots % c).int()


def _grid_prompts(coord, pred, conf, label, present, bounds, grid, threshold, status):
    """the launch; returns prompt arrays of full capacity, status[_PROMPTS] holds the count (not read here)"""
    n, c, dev = coord.shape[0], present.shape[0], coord.device
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if n == 0:
        return empty, empty
    lo_x, hi_x, lo_y, hi_y = bounds
    nx, ny = grid_cells(lo_x, hi_x, lo_y, hi_y, grid)
    if nx == 0 or ny == 0:
        return empty, empty
    if nx * ny * c >= 2 ** 31:
        raise ValueError("ao_amd refine: %d x %d cells x %d classes do not fit the prompt table" % (nx, ny, c))
    if not _use_hip():
        return _prompts_torch(coord, pred, conf, label, present, float(lo_x), float(lo_y), nx, ny, grid, threshold, status)
    L = _lib.lib()
    capacity = min(n, nx * ny * c)
    prompt_idx = torch.empty(capacity, dtype=torch.int32, device=dev)
    prompt_cls = torch.empty(capacity, dtype=torch.int32, device=dev)
    nbytes = L.refine_workspace_bytes(n, c, nx * ny, 0)
    ws = _lib.workspace(nbytes, dev)
    rc = L.refine_prompts_hip_launcher(n, c, coord.data_ptr(), pred.data_ptr(), conf.data_ptr(), label.data_ptr(),
                                       present.data_ptr(), float(lo_x), float(lo_y), nx, ny, float(grid), float(threshold),
                                       ws.data_ptr(), ws.numel(), capacity, prompt_idx.data_ptr(), prompt_cls.data_ptr(),
                                       status.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "refine_prompts_hip_launcher")
    return prompt_idx, prompt_cls


def _check_scene(coord, pred, conf, label, present):
    _lib.require_cuda(coord, pred, conf, label, present)
    n = coord.shape[0]
    c = _classes(present.shape[0])
    if tuple(coord.shape) != (n, 3) or coord.dtype != torch.float32:
        raise ValueError("ao_amd refine: coord must be (n, 3) float32, got %s %s" % (tuple(coord.shape), coord.dtype))
    if not (tuple(pred.shape) == tuple(conf.shape) == tuple(label.shape) == (n,)):
        raise ValueError("ao_amd refine: pred %s, conf %s, label %s for %d points"
                         % (tuple(pred.shape), tuple(conf.shape), tuple(label.shape), n))
    if pred.dtype != torch.int32 or label.dtype != torch.int32 or conf.dtype != torch.float32:
        raise ValueError("ao_amd refine: pred and label must be int32 and conf float32")
    if present.dim() != 1 or present.dtype not in (torch.uint8, torch.bool):
        raise ValueError("ao_amd refine: present must be (C,) uint8 or bool")
    present = present.to(torch.uint8)
    return coord.contiguous(), pred.contiguous(), conf.contiguous(), label.contiguous(), present.contiguous(), c


def grid_prompts(coord, pred, conf, label, present, grid=0.5, threshold=0.9, bounds=None):
    """One prompt per (grid cell, class): (prompt_idx, prompt_cls) int32 device tensors in the reference's order (x cell, y
    cell, class ascending).  coord (n, 3) fp32, pred / conf of scene_confidence, label (n,) int32: the current pseudo-labels,
    present (C,) uint8: which classes the scene holds.  bounds = (lo_x, hi_x, lo_y, hi_y) of coord when the caller has them
    on the host (else they are computed on the device and read back).  Reads the prompt count: one synchronisation."""
    coord, pred, conf, label, present, _ = _check_scene(coord, pred, conf, label, present)
    status = _new_status(coord.device)
    if bounds is None and coord.shape[0]:
        bounds = _xy_bounds(coord)
    prompt_idx, prompt_cls = _grid_prompts(coord, pred, conf, label, present, bounds, grid, threshold, status)
    error, count = status[:2].tolist()
    _raise_for(error)
    return prompt_idx[:count], prompt_cls[:count]


def _vote_torch(bridge, pred, conf, prompt_cls, masks, threshold, vote, status):
    p_count, height, width = masks.shape
    c = vote.shape[1]
    u, v, vis = bridge[:, 0].long(), bridge[:, 1].long(), bridge[:, 2] == 1
    bad = vis & ((u < 0) | (u > height) | (v < 0) | (v > width))
    status[_ERROR] |= torch.where(bad.any(), _BAD_PIXEL, 0).int()
    r, q = torch.where(u == 0, height - 1, u - 1), torch.where(v == 0, width - 1, v - 1)
    rows = torch.nonzero(vis & ~bad & ((r != 0) | (q != 0))).reshape(-1)
    inside = masks.reshape(p_count, -1)[:, (r * width + q)[rows]] != 0  # (P, V)
    k = pred[rows].long()
    hot = (conf[rows] > threshold) & (k >= 0) & (k < c)
    onehot = torch.nn.functional.one_hot(k.clamp(0, c - 1), c).double() * hot[:, None]
    hist = inside.double() @ onehot  # counts: exact in float64
    cast = (hist.sum(1) > 0) & (_first_argmax(hist) == prompt_cls.long())
    add = inside[cast].t().int()  # (V, casting prompts)
    cls = prompt_cls[cast].long()
    vote.index_put_((rows[:, None].expand_as(add), cls[None, :].expand_as(add)), add, accumulate=True)


class LabelRefiner:
    """One scene at a time: begin(...), vote_view(...) per view, finish().

        r = LabelRefiner(13)
        r.begin(logits, coord, label, present)          # pred, conf, prompts; r.prompt_idx / r.prompt_cls
        for bridge in views:
            r.vote_view(bridge, masks_for)              # masks_for(pixel_xy (P, 2) float32, prompt_cls (P,)) -> (P, H, W)
        label, n_updated, touched = r.finish()
    """

    def __init__(self, num_classes, grid=0.5, threshold=0.9):
        self.num_classes, self.grid, self.threshold = _classes(num_classes), float(grid), float(threshold)
        if not self.grid > 0 or not self.threshold >= 0:
            raise ValueError("ao_amd refine: grid must be positive and threshold non-negative")
        self.label = None

    def begin(self, logits, coord, label, present, bounds=None):
        """logits (n, C) fp32, coord (n, 3) fp32, label (n,) int32 (copied: the caller's tensor is not written), present
        (C,) uint8 -- device tensors.  bounds: see grid_prompts."""
        _lib.require_cuda(logits, coord, label, present)
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or present.shape[0] != self.num_classes:
            raise ValueError("LabelRefiner.begin: logits %s, present %s for %d classes"
                             % (tuple(logits.shape), tuple(present.shape), self.num_classes))
        self.pred, self.conf = scene_confidence(logits)
        coord, self.pred, self.conf, label, present, _ = _check_scene(coord, self.pred, self.conf, label, present)
        self.n = coord.shape[0]
        self.label = label.clone()
        self._status = _new_status(coord.device)
        if bounds is None and self.n:
            bounds = _xy_bounds(coord)
        prompt_idx, prompt_cls = _grid_prompts(coord, self.pred, self.conf, self.label, present, bounds, self.grid,
                                               self.threshold, self._status)
        error, count = self._status[:2].tolist()  # THE read of the scene
        _raise_for(error)
        self.prompt_idx, self.prompt_cls = prompt_idx[:count], prompt_cls[:count]
        self.vote = torch.zeros((self.n, self.num_classes), dtype=torch.int32, device=coord.device)
        self.touched = False
        return self

    def vote_view(self, bridge, masks_for):
        """bridge (n, 3) int32 / int64 (u, v, visible) of one view.  masks_for is called only when the view sees a prompt,
        with the (u, v) of the visible prompts as float32 (P, 2) and their classes (P,) int32; it returns (P, H, W) bool or
        uint8 on the device.  Returns the number of prompts the view saw."""
        _lib.require_cuda(bridge)
        if tuple(bridge.shape) != (self.n, 3):
            raise ValueError("LabelRefiner.vote_view: bridge %s for %d points" % (tuple(bridge.shape), self.n))
        if self.prompt_idx.numel() == 0:
            return 0
        if bridge.dtype != torch.int32:
            bridge = bridge.int()
        bridge = bridge.contiguous()
        at_prompts = bridge[self.prompt_idx.long()]
        seen = torch.nonzero(at_prompts[:, 2] == 1).reshape(-1)  # a read: the predictor's batch size is host-side
        p_count = seen.numel()
        if p_count == 0:
            return 0
        self.touched = True
        prompt_cls = self.prompt_cls[seen].contiguous()
        masks = masks_for(at_prompts[seen, :2].float(), prompt_cls)
        _lib.require_cuda(masks)
        if masks.dim() != 3 or masks.shape[0] != p_count or masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError("LabelRefiner.vote_view: masks_for returned %s %s for %d prompts"
                             % (tuple(masks.shape), masks.dtype, p_count))
        masks = masks.contiguous().view(torch.uint8)
        height, width = masks.shape[1:]
        if not _use_hip():
            _vote_torch(bridge, self.pred, self.conf, prompt_cls, masks, self.threshold, self.vote, self._status)
            return p_count
        L = _lib.lib()
        nbytes = L.refine_workspace_bytes(self.n, self.num_classes, 0, p_count)
        ws = _lib.workspace(nbytes, bridge.device)
        rc = L.refine_vote_hip_launcher(self.n, self.num_classes, bridge.data_ptr(), self.pred.data_ptr(), self.conf.data_ptr(),
                                        p_count, prompt_cls.data_ptr(), masks.data_ptr(), height, width, self.threshold,
                                        ws.data_ptr(), ws.numel(), self.vote.data_ptr(), self._status.data_ptr(),
                                        _lib.stream_ptr())
        _lib.check(rc, "refine_vote_hip_launcher")
        return p_count

    def finish(self, check=True):
        """(label, n_updated, touched): label (n,) int32 on the device.  touched False (the reference's flag_updated): no
        view saw a prompt and the labels are as they were.  check=True reads the status words once: raises IndexError when a
        view held a pixel outside its image (those points were skipped), and n_updated is an int; check=False reads nothing
        and n_updated is a 0-d device tensor."""
        if self.touched:
            if not _use_hip():
                result = _first_argmax(self.vote)
                pred = self.pred.long()
                valid = (self.vote.sum(1) != 0) & (result == pred) & (pred != -1)
                self._status[_UPDATED] += (valid & (self.label.long() != result)).sum().int()
                self.label = torch.where(valid, result.int(), self.label)
            else:
                rc = _lib.lib().refine_update_hip_launcher(self.n, self.num_classes, self.vote.data_ptr(), self.pred.data_ptr(),
                                                           self.label.data_ptr(), self._status.data_ptr(), _lib.stream_ptr())
                _lib.check(rc, "refine_update_hip_launcher")
        if not check:
            return self.label, self._status[_UPDATED], self.touched
        error, _, updated = self._status[:3].tolist()
        _raise_for(error)
        return self.label, updated, self.touched


def refine_scene(logits, coord, label, present, views, masks_for, grid=0.5, threshold=0.9, device=None, details=None):
    """The whole refinement of one scene.  logits (n, C): the basket's host array (or a tensor); coord (n, 3); label (n,) or
    (n, 1), any integer type, numpy or tensor; present (C,) mask of the classes the scene holds; views: iterable of
    (bridge (n, 3) integer array, view_key); masks_for(view_key, pixel_xy, prompt_cls) -> (P, H, W) device masks.  Everything
    is converted and uploaded once.  Returns (label, n_updated, touched), label in the container, shape and dtype it came in.
    details: a dict that receives the refiner's device tensors (pred, conf, prompt_idx, prompt_cls, vote) and `seen`, the
    number of prompts each view saw."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    host_coord = None if torch.is_tensor(coord) else np.ascontiguousarray(coord, dtype=np.float32)
    bounds = None
    if host_coord is not None and host_coord.shape[0]:
        lo, hi = host_coord.min(axis=0), host_coord.max(axis=0)
        bounds = (lo[0], hi[0], lo[1], hi[1])
    was_numpy = not torch.is_tensor(label)
    label_in = torch.as_tensor(label)
    to_dev = lambda a, dtype: torch.as_tensor(a).to(device=device, dtype=dtype)  # noqa: E731
    logits_d = to_dev(logits, torch.float32)
    refiner = LabelRefiner(logits_d.shape[1], grid, threshold)
    refiner.begin(logits_d, to_dev(coord if host_coord is None else host_coord, torch.float32),
                  to_dev(label_in.reshape(-1), torch.int32), to_dev(present, torch.uint8),
                  bounds=bounds)
    seen = [refiner.vote_view(to_dev(bridge, torch.int32),
                              lambda pixel_xy, prompt_cls, _key=view_key: masks_for(_key, pixel_xy, prompt_cls))
            for bridge, view_key in views]
    out, updated, touched = refiner.finish()
    if details is not None:
        details.update(pred=refiner.pred, conf=refiner.conf, prompt_idx=refiner.prompt_idx, prompt_cls=refiner.prompt_cls,
                       vote=refiner.vote, seen=seen)
    out = out.to(device=label_in.device, dtype=label_in.dtype).reshape(label_in.shape)
    return (out.numpy() if was_numpy else out), updated, touched
