"""The PP2S label pipeline on the device: bridges between a room's points and its camera views, one weak label per instance,
and the propagation of those labels through the mask predictor's masks.

Reference (three stand-alone numpy scripts, run once per room before any training):

    pointcept/utils/my_make_bridge_final.py:88-96     the room's alignment (an angle and a centre per room)
                                           :122-153   per view: every point projected by K * RT, np.round, the image bounds,
                                                      a depth-image lookup, |depth - z_cam| < 0.1; a uint16 (x, y, 1) row per
                                                      visible point
    my_choose_weak_label_final.py:59-88               one labelled point per instance: the middle visible one in index order,
                                                      the middle one of the instance when no view sees it
    my_run_sam_final.py:83-114                        per view, per weak point visible in it: one mask; a python loop over
                                                      every visible point of the view; a point that collected one class keeps
                                                      it, one that collected several becomes -1
                       :47-60, :117-122               the weak points are written over with their ground truth

Here each stage is a launch of ao_amd/csrc/pp2s.hip (C ABI: include/ptv2_pp2s_hip.h).  The mask predictor is NOT part of this
module: `masks_for` is the caller's (SAM in the reference), and so is all file I/O.  The scripts' quirks are kept as they are
(DESIGN.md section 9): the bounds named `height` and `width` the other way round, no test for points behind the camera,
`mask[y - 1][x - 1]` with python's wrap of index -1, `mask[0][0]` not cleared.

Host synchronisations: `project_view`, `choose_weak_labels`, `vote_view` and `finish(check=False)` read nothing;
`LabelPropagator(...)` reads the indices of the weak points once, `view_prompts` reads their bridge rows once per view,
`pp2s_scene` also reads the visible counts of all views once.

There is no CPU fallback.  AO_AMD_PP2S=torch runs the same contracts in eager torch on the device (the A/B path, as
AO_AMD_REFINE=torch).
"""
import os

import numpy as np
import torch

from .. import _abi, _lib

_K = _abi.pp2s_consts
MIN_C, MAX_C, MAX_BOUND = _K["PTV2_PP2S_MIN_C"], _K["PTV2_PP2S_MAX_C"], _K["PTV2_PP2S_MAX_BOUND"]
_ERROR, _VISIBLE = _K["PTV2_PP2S_STATUS_ERROR"], _K["PTV2_PP2S_STATUS_VISIBLE"]
_BAD_PIXEL, _BAD_CLASS = _K["PTV2_PP2S_BAD_PIXEL"], _K["PTV2_PP2S_BAD_CLASS"]


def _use_hip():
    return os.environ.get("AO_AMD_PP2S", "hip") != "torch"


def new_status(device):
    """the zeroed status words the launches of one room share (include/ptv2_pp2s_hip.h)"""
    return torch.zeros(_K["PTV2_PP2S_STATUS_WORDS"], dtype=torch.int32, device=device)


def raise_for_status(status):
    """reads the error word: IndexError for a set PTV2_PP2S_BAD_* bit"""
    error = int(status[_ERROR])
    if error & _BAD_PIXEL:
        raise IndexError("ao_amd pp2s: a pixel outside its image (a projection outside the depth image, or a bridge row "
                         "outside the masks); the point was skipped")
    if error & _BAD_CLASS:
        raise IndexError("ao_amd pp2s: a prompt class outside the class range; the prompt was skipped")


def _workspace(n, height, width, device):
    nbytes = _lib.lib().pp2s_workspace_bytes(n, height, width)
    if nbytes < 0:
        raise ValueError("ao_amd pp2s: no workspace for %d points and a %d x %d image" % (n, height, width))
    return _lib.workspace(nbytes, device)


def rotation(angle_deg):
    """(cos, sin) of my_make_bridge_final.py:90-92 for a room's alignment angle in degrees, in the script's arithmetic"""
    angle = 360 - angle_deg
    angle = (2 - angle / 180) * np.pi
    return float(np.cos(angle)), float(np.sin(angle))


def _fma(a, b, c):
    """a * b + c with one rounding, from float64 sums and products alone (Dekker's product, Knuth's sum; the last two sums
    round twice, which differs from a fused multiply-add only on ties about 1e-16 of the elements away).  The A/B path's
    stand-in for the kernel's __fma_rn."""
    def split(x):
        t = 134217729.0 * x  # 2 ** 27 + 1
        hi = t - (t - x)
        return hi, x - hi

    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl  # a * b == p + e
    s = p + c
    v = s - p
    r = (p - (s - v)) + (c - v)                        # p + c == s + r
    return s + (r + e)


def align_room(coord, angle_deg, center):
    """coord (n, 3) float32 on the device -> the aligned room (n, 3) float64: (coord - center) rounded to float32, rotated
    about z by the room's angle and moved back, in float64 (my_make_bridge_final.py:88-96)."""
    _lib.require_cuda(coord)
    if coord.dim() != 2 or coord.shape[1] != 3 or coord.dtype != torch.float32:
        raise ValueError("ao_amd pp2s: coord must be (n, 3) float32, got %s %s" % (tuple(coord.shape), coord.dtype))
    cx, cy, cz = (float(v) for v in np.asarray(center, np.float64).reshape(3))
    rot_cos, rot_sin = rotation(angle_deg)
    coord = coord.contiguous()
    n = coord.shape[0]
    if not _use_hip():
        t = (coord.double() - torch.tensor([cx, cy, cz], dtype=torch.float64, device=coord.device)).float().double()
        c, s = (torch.tensor(v, dtype=torch.float64, device=coord.device) for v in (rot_cos, rot_sin))
        return torch.stack([_fma(t[:, 1], -s, t[:, 0] * c) + cx, _fma(t[:, 1], c, t[:, 0] * s) + cy, t[:, 2] + cz], 1)
    out = torch.empty((n, 3), dtype=torch.float64, device=coord.device)
    rc = _lib.lib().pp2s_align_hip_launcher(n, coord.data_ptr(), cx, cy, cz, rot_cos, rot_sin, out.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "pp2s_align_hip_launcher")
    return out


def _project_torch(coord64, krt, rt, depth, height, width, tol, seen_any, status):
    x, y, z = coord64.unbind(1)

    def row(m, r):
        return ((float(m[r, 0]) * x + float(m[r, 1]) * y) + float(m[r, 2]) * z) + float(m[r, 3])

    pz = row(krt, 2)
    rx, ry = torch.round(row(krt, 0) / pz), torch.round(row(krt, 1) / pz)  # half to even, as np.round
    valid = (rx > 0) & (ry > 0) & (rx < height) & (ry < width)
    bx, by = torch.where(valid, rx, 0.0).long(), torch.where(valid, ry, 0.0).long()
    inside = valid & (bx < depth.shape[1]) & (by < depth.shape[0])
    status[_ERROR] |= torch.where((valid & ~inside).any(), _BAD_PIXEL, 0).int()
    d = depth.reshape(-1)[torch.where(inside, by * depth.shape[1] + bx, 0)]
    visible = inside & ((d - row(rt, 2)).abs() < tol)
    status[_VISIBLE] += visible.sum().int()
    if seen_any is not None:
        seen_any |= visible.to(seen_any.dtype)
    return (torch.stack([bx, by, torch.ones_like(bx)], 1) * visible[:, None]).int()


def project_view(coord64, k_matrix, rt_matrix, depth, depth_scale=512.0, tol=0.1, seen_any=None, status=None):
    """One view's bridge.  coord64 (n, 3) float64 on the device (align_room's output); k_matrix (3, 3) and rt_matrix (3, 4)
    host arrays, K * RT is formed on the host with np.matmul as the reference does; depth (H, W) on the device: the raw
    integer image (divided by depth_scale in float64, as np.array(png) / 512) or a float64 image with depth_scale=1.
    Returns (bridge, n_visible): bridge (n, 3) int32 = (x, y, 1) for the visible points, zeros otherwise (what
    LabelRefiner.vote_view and LabelPropagator take; bridge_to_numpy gives the file); n_visible a 0-d int32 device tensor --
    the reference saves no bridge for a view whose count is 0.  seen_any (n,) uint8: or-ed with the visible points.
    status: the room's status words (new_status); a projection outside the depth image is skipped and recorded there
    (raise_for_status, LabelPropagator.finish).  Reads nothing back."""
    _lib.require_cuda(coord64, depth, seen_any, status)
    if coord64.dim() != 2 or coord64.shape[1] != 3 or coord64.dtype != torch.float64:
        raise ValueError("ao_amd pp2s: coord64 must be (n, 3) float64, got %s %s" % (tuple(coord64.shape), coord64.dtype))
    k = np.asarray(k_matrix, np.float64)
    rt = np.asarray(rt_matrix, np.float64)
    if k.shape != (3, 3) or rt.shape != (3, 4) or depth.dim() != 2 or depth.numel() == 0:
        raise ValueError("ao_amd pp2s: k_matrix (3, 3), rt_matrix (3, 4) and a depth image (H, W), got %s, %s, %s"
                         % (k.shape, rt.shape, tuple(depth.shape)))
    krt = np.matmul(k, rt)
    height, width = float(k[0, 2] * 2 - 1), float(k[1, 2] * 2 - 1)
    if not (height <= MAX_BOUND and width <= MAX_BOUND):
        raise ValueError("ao_amd pp2s: image bounds %g x %g do not fit the bridge's uint16" % (height, width))
    n, dev = coord64.shape[0], coord64.device
    if seen_any is not None and (tuple(seen_any.shape) != (n,) or seen_any.dtype != torch.uint8):
        raise ValueError("ao_amd pp2s: seen_any must be (n,) uint8")
    if depth.dtype != torch.float64 or depth_scale != 1:
        depth = depth.double() / float(depth_scale)
    depth = depth.contiguous()
    coord64 = coord64.contiguous()
    shared = status is not None
    if shared:
        status[_VISIBLE:_VISIBLE + 1].zero_()
    else:
        status = new_status(dev)
    if not _use_hip():
        bridge = _project_torch(coord64, krt, rt, depth, height, width, float(tol), seen_any, status)
    else:
        bridge = torch.empty((n, 3), dtype=torch.int32, device=dev)
        rc = _lib.lib().pp2s_project_hip_launcher(n, coord64.data_ptr(), *[float(v) for v in krt.reshape(-1)],
                                                  *[float(v) for v in rt.reshape(-1)], depth.data_ptr(), depth.shape[0],
                                                  depth.shape[1], height, width, float(tol), bridge.data_ptr(),
                                                  _lib.ptr(seen_any), status.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pp2s_project_hip_launcher")
    return bridge, (status[_VISIBLE].clone() if shared else status[_VISIBLE])


def bridge_to_numpy(bridge):
    """the (n, 3) uint16 array my_make_bridge_final.py saves for a view (a read)"""
    return bridge.cpu().numpy().astype(np.uint16)


def _weak_torch(instance, seen_any):
    n = instance.shape[0]
    weak = torch.zeros(n, dtype=torch.uint8, device=instance.device)
    if n == 0:
        return weak
    order = torch.argsort(instance, stable=True)  # by instance, ascending index inside one
    _, counts = torch.unique_consecutive(instance[order], return_counts=True)
    end = torch.cumsum(counts, 0)
    start = end - counts
    flags = (seen_any[order] != 0).long()
    seen = torch.cumsum(flags, 0)
    before = seen[start] - flags[start]
    count_seen = seen[end - 1] - before
    at_seen = torch.searchsorted(seen, before + count_seen // 2 + 1)  # the first position whose sum reaches the target
    at = torch.where(count_seen > 0, at_seen.clamp(max=n - 1), start + counts // 2)
    weak[order[at]] = 1
    return weak


def choose_weak_labels(instance, seen_any):
    """instance (n,) int32 (any values; -1 is an instance like any other), seen_any (n,) uint8 -> weak (n,) uint8: one point
    per instance, the seen point of rank count_seen // 2 among its seen points in index order, or the point of rank
    count // 2 when no view sees the instance (my_choose_weak_label_final.py:71-88).  Reads nothing back."""
    _lib.require_cuda(instance, seen_any)
    n = instance.shape[0]
    if instance.dim() != 1 or instance.dtype != torch.int32 or tuple(seen_any.shape) != (n,) or seen_any.dtype != torch.uint8:
        raise ValueError("ao_amd pp2s: instance must be (n,) int32 and seen_any (n,) uint8")
    instance, seen_any = instance.contiguous(), seen_any.contiguous()
    if not _use_hip():
        return _weak_torch(instance, seen_any)
    weak = torch.empty(n, dtype=torch.uint8, device=instance.device)
    if n == 0:
        return weak
    ws = _workspace(n, 0, 0, instance.device)
    rc = _lib.lib().pp2s_weak_hip_launcher(n, instance.data_ptr(), seen_any.data_ptr(), weak.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "pp2s_weak_hip_launcher")
    return weak


class LabelPropagator:
    """One room at a time: view_prompts(...) and vote_view(...) per saved view, finish().

        p = LabelPropagator(semantic_gt, weak, 13)
        for key, bridge in views:
            idx, xy, cls = p.view_prompts(bridge)            # host arrays: the weak points this view sees
            if len(idx):
                p.vote_view(bridge, predictor(key, xy), cls) # (P, H, W) masks on the device, one per prompt
        labels = p.finish()

    semantic_gt (n,) or (n, 1) integer, weak (n,) uint8 -- device tensors.  The constructor reads the indices of the weak
    points that are prompts (weak != 0, ground truth != -1) once."""

    def __init__(self, semantic_gt, weak, num_classes, status=None):
        _lib.require_cuda(semantic_gt, weak, status)
        self.num_classes = int(num_classes)
        if not MIN_C <= self.num_classes <= MAX_C:
            raise ValueError("ao_amd pp2s: %d classes, supported are %d..%d" % (self.num_classes, MIN_C, MAX_C))
        self.gt = semantic_gt.reshape(-1).int().contiguous()
        self.n = self.gt.shape[0]
        if tuple(weak.shape) != (self.n,) or weak.dtype not in (torch.uint8, torch.bool):
            raise ValueError("ao_amd pp2s: weak must be (n,) uint8 for %d points, got %s %s" % (self.n, tuple(weak.shape), weak.dtype))
        self.weak = weak.to(torch.uint8).contiguous()
        self.status = new_status(self.gt.device) if status is None else status
        self.seen_bits = torch.zeros(self.n, dtype=torch.int32, device=self.gt.device)  # a uint32 per point, one bit per class
        self.prompt_rows = torch.nonzero((self.weak != 0) & (self.gt != -1)).reshape(-1)  # THE read of the room
        self.label = None

    def _bridge(self, bridge):
        _lib.require_cuda(bridge)
        if tuple(bridge.shape) != (self.n, 3):
            raise ValueError("LabelPropagator: bridge %s for %d points" % (tuple(bridge.shape), self.n))
        return (bridge if bridge.dtype == torch.int32 else bridge.int()).contiguous()

    def view_prompts(self, bridge):
        """(idx (P,) int64, xy (P, 2) int32, cls (P,) int32), numpy, in index order: the weak points with bridge[p][2] != 0,
        their (x, y) pixels (what the predictor takes as point_coords) and their ground truth (my_run_sam_final.py:87-96).
        One read."""
        bridge = self._bridge(bridge)
        rows = self.prompt_rows
        if rows.numel() == 0:
            return np.zeros(0, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
        table = torch.cat([bridge[rows], self.gt[rows, None], rows[:, None].int()], 1).cpu().numpy()
        table = table[table[:, 2] != 0]
        return table[:, 4].astype(np.int64), table[:, :2].astype(np.int32), table[:, 3].astype(np.int32)

    def vote_view(self, bridge, masks, prompt_cls):
        """masks (P, H, W) bool or uint8 on the device, one per prompt of view_prompts; prompt_cls (P,) their classes (a
        device tensor is not read; a host array is uploaded).  Every visible point (bridge[i][2] == 1) collects the classes
        of the masks that hold its element [y - 1][x - 1].  Returns P.  Reads nothing back."""
        bridge = self._bridge(bridge)
        _lib.require_cuda(masks)
        prompt_cls = torch.as_tensor(prompt_cls).to(device=bridge.device, dtype=torch.int32).reshape(-1).contiguous()
        p_count = prompt_cls.shape[0]
        if masks.dim() != 3 or masks.shape[0] != p_count or masks.dtype not in (torch.bool, torch.uint8):
            raise ValueError("LabelPropagator.vote_view: masks %s %s for %d prompts" % (tuple(masks.shape), masks.dtype, p_count))
        if p_count == 0 or self.n == 0:
            return p_count
        height, width = masks.shape[1:]
        if height == 0 or width == 0:
            raise ValueError("LabelPropagator.vote_view: masks without pixels")
        masks = masks.contiguous().view(torch.uint8)
        if not _use_hip():
            self._vote_torch(bridge, masks, prompt_cls)
            return p_count
        L = _lib.lib()
        ws = _workspace(0, height, width, bridge.device)
        rc = L.pp2s_pixel_labels_hip_launcher(p_count, self.num_classes, prompt_cls.data_ptr(), masks.data_ptr(), height, width,
                                              ws.data_ptr(), ws.numel(), self.status.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pp2s_pixel_labels_hip_launcher")
        rc = L.pp2s_vote_hip_launcher(self.n, bridge.data_ptr(), height, width, ws.data_ptr(), ws.numel(),
                                      self.seen_bits.data_ptr(), self.status.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pp2s_vote_hip_launcher")
        return p_count

    def _vote_torch(self, bridge, masks, prompt_cls):
        p_count, height, width = masks.shape
        ok = (prompt_cls >= 0) & (prompt_cls < self.num_classes)
        bit = torch.where(ok, torch.ones_like(prompt_cls).long() << prompt_cls.clamp(0, 31).long(), 0)  # int64: bit 31 is positive
        self.status[_ERROR] |= torch.where((~ok).any(), _BAD_CLASS, 0).int()
        pixbits = torch.zeros(height * width, dtype=torch.int64, device=masks.device)
        for p in range(p_count):  # (the A/B path: clarity over speed)
            pixbits |= torch.where(masks[p].reshape(-1) != 0, bit[p], 0)
        u, v, vis = bridge[:, 0].long(), bridge[:, 1].long(), bridge[:, 2] == 1
        bad = vis & ((u < 0) | (u > width) | (v < 0) | (v > height))
        self.status[_ERROR] |= torch.where(bad.any(), _BAD_PIXEL, 0).int()
        row, col = torch.where(v == 0, height - 1, v - 1), torch.where(u == 0, width - 1, u - 1)
        take = vis & ~bad
        got = torch.where(take, pixbits[torch.where(take, row * width + col, 0)], 0)
        have = self.seen_bits.long() & 0xFFFFFFFF
        both = have | got
        self.seen_bits = torch.where(both >= 2 ** 31, both - 2 ** 32, both).int()

    def finish(self, check=True):
        """label (n,) int32 on the device: the one class a point collected, -1 for none or several; the weak points whose
        ground truth is not -1 carry that ground truth.  check=True reads the status word and raises IndexError when a point
        or a prompt was skipped (a pixel outside its image, a class outside the range); check=False reads nothing."""
        if not _use_hip():
            bits = self.seen_bits.long() & 0xFFFFFFFF
            single = (bits != 0) & ((bits & (bits - 1)) == 0)
            index = torch.zeros_like(bits)
            for k in range(32):
                index = torch.where(bits == (1 << k), k, index)
            label = torch.where(single, index, -1).int()
            self.label = torch.where((self.weak != 0) & (self.gt != -1), self.gt, label)
        else:
            self.label = torch.empty(self.n, dtype=torch.int32, device=self.gt.device)
            rc = _lib.lib().pp2s_labels_hip_launcher(self.n, self.seen_bits.data_ptr(), self.weak.data_ptr(), self.gt.data_ptr(),
                                                     self.label.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "pp2s_labels_hip_launcher")
        if check:
            raise_for_status(self.status)
        return self.label


def pp2s_scene(coord, instance, semantic_gt, views, masks_for, num_classes=13, angle_deg=None, center=None, depth_scale=512.0,
               tol=0.1, device=None, details=None):
    """The whole pipeline of one room.  coord (n, 3) float32, instance and semantic_gt (n,) or (n, 1) integer: numpy arrays
    or tensors, uploaded once.  views: iterable of (view_key, k_matrix, rt_matrix, depth); depth a host or device image
    (see project_view).  angle_deg / center: the room's alignment (both or neither; without them coord is taken as aligned).
    masks_for(view_key, xy (P, 2) int32, cls (P,) int32) -> (P, H, W) device masks, one per prompt: the caller's SAM.
    A view that sees no point is dropped, as the reference saves no bridge for it.  Returns the labels as a (n, 1) int32
    numpy array (what my_run_sam_final.py saves).  details: a dict that receives coord64, bridges {view_key: tensor},
    visible {view_key: count} (every view), seen_any, weak, prompts {view_key: (idx, xy, cls)} and label (the device tensor)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    to_dev = lambda a, dtype=None: torch.as_tensor(a).to(device=device, dtype=dtype)  # noqa: E731
    if (angle_deg is None) != (center is None):
        raise ValueError("pp2s_scene: angle_deg and center go together")
    coord_d = to_dev(coord)
    if angle_deg is not None:
        coord64 = align_room(coord_d.float(), angle_deg, center)
    else:
        coord64 = coord_d.double()
    n = coord64.shape[0]
    status = new_status(device)
    seen_any = torch.zeros(n, dtype=torch.uint8, device=device)
    keys, bridges, counts = [], [], []
    for key, k_matrix, rt_matrix, depth in views:
        bridge, count = project_view(coord64, k_matrix, rt_matrix, to_dev(depth), depth_scale, tol, seen_any, status)
        keys.append(key)
        bridges.append(bridge)
        counts.append(count)
    counts = torch.stack(counts).tolist() if counts else []
    weak = choose_weak_labels(to_dev(instance).reshape(-1).int(), seen_any)
    prop = LabelPropagator(to_dev(semantic_gt), weak, num_classes, status)
    prompts = {}
    for key, bridge, count in zip(keys, bridges, counts):
        if count == 0:
            continue
        idx, xy, cls = prop.view_prompts(bridge)
        prompts[key] = (idx, xy, cls)
        if idx.size:
            prop.vote_view(bridge, masks_for(key, xy, cls), cls)
    label = prop.finish()
    if details is not None:
        details.update(coord64=coord64, bridges={k: b for k, b, c in zip(keys, bridges, counts) if c}, visible=dict(zip(keys, counts)),
                       seen_any=seen_any, weak=weak, prompts=prompts, label=label)
    return label.cpu().numpy().astype(np.int32).reshape(n, 1)
