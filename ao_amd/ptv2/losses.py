"""LovaszLoss(mode="multiclass") of the reference (pointcept/models/losses/lovasz.py:211-253) for (N, C) point logits.

Three PT-v2m2 configs train with cross-entropy plus this loss (configs/scannet/semseg-pt-v2m2-3-lovasz.py:37-40,
configs/scannet200/semseg-pt-v2m2-2-lovasz.py:43, configs/semantic_kitti/semseg-pt-v2m2-1-benchmark-submit.py:65), all with
`dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)`.  The reference runs `labels.unique()` (a host
synchronisation) and then one full `torch.sort` plus ~10 small launches per present class; here CUDA logits go through
ao_amd/csrc/lovasz.hip (18 launches forward, 1 backward, whatever the number of classes, no synchronisation).  Other inputs
(CPU tensors) take `_lovasz_softmax_torch` below, a vectorised eager formulation of the same contract; AO_AMD_LOVASZ=torch
selects it on the GPU too (an A/B switch).

Semantics (lovasz.py with per_image=False): p = softmax(logits) in fp32 (also under autocast); rows with label != ignore_index
(every row for ignore_index=None); the classes present among them, ascending, limited to `class_seen` when given; for each,
the errors |fg - p_c| sorted descending -- ties in ascending row order, which the reference leaves to torch.sort and this
package pins (a stable sort) -- dotted with _lovasz_grad; the mean over those classes, times loss_weight.  Edge cases: no class
to average (no labelled row, or none in class_seen) -> a 0-dim zero with a zero gradient (the reference returns `0`, or a
(0, C) tensor when no row is labelled); a label neither ignore_index nor in [0, C) -> NaN, and AO_AMD_CHECK_LABELS=1 raises
instead; C == 1 -> ValueError (lovasz.py:135-137); 2^24 rows or more -> ValueError (fp32 counts stop being exact)."""
import os

import torch
import torch.nn as nn

MAX_ROWS = 1 << 24
_SEEN_CACHE = {}


def _seen_mask(class_seen, c, device):
    """int32 (C,) device mask of class_seen, built once per (classes, C, device): a host-to-device copy per step would be a
    synchronisation."""
    key = (tuple(int(v) for v in class_seen), c, str(device))
    m = _SEEN_CACHE.get(key)
    if m is None:
        host = torch.zeros(c, dtype=torch.int32)
        for v in key[0]:
            if 0 <= v < c:
                host[v] = 1
        m = host.to(device)
        _SEEN_CACHE[key] = m
    return m


def _check_shape(logits):
    if logits.dim() != 2:
        raise ValueError("lovasz_softmax: logits must be (N, C), got %s" % (tuple(logits.shape),))
    n, c = logits.shape
    if c == 1:
        raise ValueError("Sigmoid output possible only with 1 class")  # lovasz.py:135-137
    if n >= MAX_ROWS:
        raise ValueError("lovasz_softmax: %d rows; at most %d (the fp32 cumulative counts of the reference stop being exact)"
                         % (n, MAX_ROWS - 1))


class _LovaszSoftmax(torch.autograd.Function):
    """ao_amd/csrc/lovasz.hip on fp32 CUDA logits (N, C), int64 labels."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, label, ignore_index, seen, weight):
        from .. import _lib

        logits, label = logits.contiguous(), label.contiguous()
        n, c = logits.shape
        L = _lib.lib()
        dev = logits.device
        out = torch.empty(4, dtype=torch.float32, device=dev)  # loss, classes averaged, bad labels, rows used
        saved = torch.empty(L.lovasz_softmax_saved_bytes(n, c), dtype=torch.uint8, device=dev)
        ws = _lib.workspace(L.lovasz_softmax_workspace_bytes(n, c), dev)
        rc = L.lovasz_softmax_forward_hip_launcher(
            n, c, logits.data_ptr(), label.data_ptr(), 0 if ignore_index is None else int(ignore_index),
            0 if ignore_index is None else 1, _lib.ptr(seen), float(weight), out.data_ptr(), saved.data_ptr(), saved.numel(),
            ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "lovasz_softmax_forward_hip_launcher")
        if os.environ.get("AO_AMD_CHECK_LABELS") == "1" and float(out[2]) > 0:  # costs a synchronisation: debugging aid
            raise ValueError("lovasz_softmax: %d labels are neither ignore_index=%s nor in [0, %d)"
                             % (int(out[2]), ignore_index, c))
        ctx.save_for_backward(logits, saved)
        ctx.weight = float(weight)
        return out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        from .. import _lib

        logits, saved = ctx.saved_tensors
        n, c = logits.shape
        g = g.contiguous().float()
        gl = torch.empty_like(logits)
        rc = _lib.lib().lovasz_softmax_backward_hip_launcher(n, c, logits.data_ptr(), saved.data_ptr(), ctx.weight,
                                                             g.data_ptr(), gl.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "lovasz_softmax_backward_hip_launcher")
        return gl, None, None, None, None


def _lovasz_softmax_torch(logits, label, ignore_index=-1, class_seen=None, weight=1.0):
    """The same contract in eager torch, every class at once: ignored rows get the error -1 (they sort last and are masked
    out), each column is sorted with a stable descending sort, and the classes not averaged are masked out of the mean.
    No host synchronisation either; autograd differentiates through the sorted values (the permutation is a constant)."""
    n, c = logits.shape
    p = torch.softmax(logits.float(), dim=1)
    label = label.reshape(-1)
    used = torch.ones_like(label, dtype=torch.bool) if ignore_index is None else label != ignore_index
    in_range = (label >= 0) & (label < c)
    bad = used & ~in_range
    used = used & in_range
    fg = torch.nn.functional.one_hot(torch.where(used, label, torch.zeros_like(label)), c).to(p.dtype) * used[:, None]
    errors = torch.where(used[:, None], (fg - p).abs(), torch.full_like(p, -1.0))
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
    fg_sorted = torch.gather(fg, 0, perm)
    used_sorted = torch.gather(used[:, None].expand(n, c).to(p.dtype), 0, perm)
    gts = fg.sum(0)
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (used_sorted - fg_sorted).cumsum(0)  # ignored rows are all behind the used ones
    jac = 1.0 - inter / union.clamp_min(1.0)
    grad = torch.cat([jac[:1], jac[1:] - jac[:-1]], 0) * used_sorted
    per_class = (errors_sorted * used_sorted * grad).sum(0)
    keep = gts > 0
    if class_seen is not None:
        keep = keep & _seen_mask(class_seen, c, p.device).bool()
    count = keep.sum()
    loss = (per_class * keep).sum() / count.clamp_min(1).to(p.dtype) * weight
    return torch.where(bad.any(), torch.full_like(loss, float("nan")), loss)


def lovasz_softmax(logits, label, ignore_index=-1, class_seen=None, loss_weight=1.0):
    """LovaszLoss(mode="multiclass", per_image=False, ignore_index, class_seen, loss_weight)(logits, label) for (N, C)
    logits: the HIP kernels for CUDA logits, the eager formulation otherwise (or with AO_AMD_LOVASZ=torch)."""
    _check_shape(logits)
    n, c = logits.shape
    native = logits.is_cuda and os.environ.get("AO_AMD_LOVASZ", "hip") != "torch"
    if native and n > 0 and c <= 1024:
        if label.dtype != torch.int64:
            label = label.long()
        seen = None if class_seen is None else _seen_mask(class_seen, c, logits.device)
        return _LovaszSoftmax.apply(logits, label, ignore_index, seen, float(loss_weight))
    if n == 0:
        return logits.sum() * 0.0
    loss = _lovasz_softmax_torch(logits, label, ignore_index, class_seen, float(loss_weight))
    if os.environ.get("AO_AMD_CHECK_LABELS") == "1":
        lab = label.reshape(-1)
        used = torch.ones_like(lab, dtype=torch.bool) if ignore_index is None else lab != ignore_index
        nbad = int((used & ((lab < 0) | (lab >= c))).sum())
        if nbad:
            raise ValueError("lovasz_softmax: %d labels are neither ignore_index=%s nor in [0, %d)" % (nbad, ignore_index, c))
    return loss


class LovaszLoss(nn.Module):
    """The reference's constructor (lovasz.py:213-241).  Only mode="multiclass" with per_image=False is implemented: it is
    the form every PT-v2m2 config uses; the binary / multilabel hinge modes are not on this path, and per_image on an
    (N, C) point tensor would mean one "image" per point."""

    def __init__(self, mode, class_seen=None, per_image=False, ignore_index=None, loss_weight=1.0):
        super().__init__()
        if mode not in ("binary", "multiclass", "multilabel"):
            raise ValueError("Wrong mode {}.".format(mode))
        if mode != "multiclass":
            raise NotImplementedError("LovaszLoss(mode=%r): only mode='multiclass' is implemented (no PT-v2m2 config uses "
                                      "the binary / multilabel hinge modes)" % mode)
        if per_image:
            raise NotImplementedError("LovaszLoss(per_image=True): not implemented (no PT-v2m2 config uses it, and on (N, C) "
                                      "point logits an image would be one point)")
        self.mode = mode
        self.class_seen = None if class_seen is None else [int(v) for v in class_seen]
        self.per_image = False
        self.ignore_index = ignore_index
        self.loss_weight = float(loss_weight)

    def forward(self, y_pred, y_true):
        return lovasz_softmax(y_pred, y_true, self.ignore_index, self.class_seen, self.loss_weight)
