"""PointGroup's operators on ao_amd/csrc/pointgroup.hip (C ABI include/ptv2_pg_hip.h).

`ballquery_batch_p` and `bfs_cluster` keep the signatures and return values of the reference's libs/pointgroup_ops (put
`dropin/` on the path and `import pointgroup_ops` resolves to this module).  `ball_query`, `cluster`, `proposals` and
`bias_loss` are what ao_amd/pointgroup/model.py calls: the same stages without the trip through the host.

AO_AMD_PG=torch (read on every call) is the A/B path: the ball query as chunked eager torch on the device, the clustering
through the host search always, scores and losses as the reference's eager statements.
"""
import ctypes
import os

import torch

from .. import _abi, _lib

BALL_CAP = _abi.pg_consts["PG_BALL_CAP"]
MAX_CLOUDS = _abi.pg_consts["PG_MAX_CLOUDS"]
MAX_CLASSES = _abi.pg_consts["PG_MAX_CLASSES"]
_TORCH_CHUNK = 1024  # rows of one eager distance block


def use_hip():
    return os.environ.get("AO_AMD_PG", "hip") != "torch"


def _csr(idx, start_len):
    return _abi.pg_structs["pg_csr"](_lib.ptr(idx) or None, start_len.data_ptr(), idx.numel())


# ------------------------------------------------------------------------------------------------------- ball query ----
def _ball_query_torch(coords, offsets, radius):
    n = coords.shape[0]
    r2 = torch.tensor(float(radius), dtype=torch.float32, device=coords.device) ** 2
    bounds = offsets.tolist()
    lens, lists, capped = torch.zeros(n, dtype=torch.int32, device=coords.device), [], False
    for s in range(len(bounds) - 1):
        lo, hi = bounds[s], bounds[s + 1]
        seg = coords[lo:hi]
        for at in range(lo, hi, _TORCH_CHUNK):
            q = coords[at:min(at + _TORCH_CHUNK, hi)]
            d = q[:, None, :] - seg[None, :, :]
            hit = (d * d).sum(-1) < r2
            rank = hit.cumsum(1)
            capped = capped or bool((rank[:, -1] > BALL_CAP).any())
            hit &= rank <= BALL_CAP  # the first BALL_CAP in ascending index
            lens[at:at + q.shape[0]] = hit.sum(1)
            lists.append(hit.nonzero()[:, 1].int() + lo)  # (row-major: ascending index within a row)
    idx = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.int32, device=coords.device)
    start = lens.cumsum(0, dtype=torch.int32) - lens
    return idx, torch.stack([start, lens], 1).contiguous(), capped


def ball_query(coords, batch_offsets, radius):
    """(idx (nActive) int32, start_len (n, 2) int32, capped bool) of coords (n, 3) fp32 and batch_offsets (B + 1) int32: for
    point p the ascending indices k of its segment with d2(p, k) < radius^2 (p included), the first BALL_CAP of them;
    start the exclusive prefix sum of len in point order; capped: some point had a (BALL_CAP + 1)-th neighbour."""
    _lib.require_cuda(coords, batch_offsets)
    if coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.float32:
        raise ValueError("ao_amd pointgroup: coords must be (n, 3) float32, got %s %s" % (tuple(coords.shape), coords.dtype))
    n, b = coords.shape[0], batch_offsets.numel() - 1
    if batch_offsets.dim() != 1 or not 1 <= b <= MAX_CLOUDS or not float(radius) > 0:
        raise ValueError("ao_amd pointgroup: %d segments (1..%d), radius %r (> 0)" % (b, MAX_CLOUDS, radius))
    dev = coords.device
    coords, offsets = coords.contiguous(), batch_offsets.int().contiguous()
    if n == 0:
        return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev), False)
    if not use_hip():
        return _ball_query_torch(coords, offsets, radius)
    L = _lib.lib()
    # (a buffer of its own: the fill pass reads the grid the count pass left in it)
    ws = torch.empty(L.ptv2_pg_ballquery_workspace_bytes(n, b), dtype=torch.uint8, device=dev)
    start_len = torch.empty((n, 2), dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)  # nActive, capped
    rc = L.pg_ballquery_count_hip_launcher(n, b, coords.data_ptr(), offsets.data_ptr(), float(radius), start_len.data_ptr(),
                                           meta.data_ptr(), meta.data_ptr() + 4, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "pg_ballquery_count_hip_launcher")
    n_active, capped = meta.tolist()  # the read-back that sizes the lists exactly
    idx = torch.empty(n_active, dtype=torch.int32, device=dev)
    rc = L.pg_ballquery_fill_hip_launcher(n, b, coords.data_ptr(), offsets.data_ptr(), float(radius), start_len.data_ptr(),
                                          n_active, _lib.ptr(idx) if n_active else 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "pg_ballquery_fill_hip_launcher")
    return idx, start_len, bool(capped)


def ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive):
    """libs/pointgroup_ops: (idx (nActive) int32, start_len (n, 2) int32).  `meanActive` sized the reference's guessed buffer
    and is unused: the lists are counted before they are written.  `batch_idxs` is implied by `batch_offsets`."""
    _lib.require_cuda(coords, batch_idxs, batch_offsets)
    idx, start_len, _ = ball_query(coords, batch_offsets, radius)
    return idx, start_len


# ------------------------------------------------------------------------------------------------------- clustering ----
def bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold):
    """libs/pointgroup_ops, CPU tensors as there: (cluster_idxs (sumNPoint, 2) int32 rows of (cluster, point) in the order of
    the reference's search, cluster_offsets (nCluster + 1) int32)."""
    for name, t in (("semantic_label", semantic_label), ("ball_query_idxs", ball_query_idxs), ("start_len", start_len)):
        if t.is_cuda:
            raise RuntimeError("ao_amd pointgroup: bfs_cluster takes CPU tensors as the reference's (%s is on %s); the device "
                               "form is ao_amd.pointgroup.cluster" % (name, t.device))
    label = semantic_label.int().contiguous()
    idx, start_len = ball_query_idxs.int().contiguous(), start_len.int().contiguous()
    n = start_len.shape[0]
    if label.numel() != n or start_len.dim() != 2 or start_len.shape[1] != 2:
        raise ValueError("ao_amd pointgroup: %d labels for start_len %s" % (label.numel(), tuple(start_len.shape)))
    rows = torch.zeros((max(n, 1), 2), dtype=torch.int32)
    offsets = torch.zeros(n + 1, dtype=torch.int32)
    count = ctypes.c_int(0)
    csr = _csr(idx, start_len)
    total = _lib.lib().pg_bfs_cluster_host(n, label.data_ptr(), ctypes.addressof(csr), int(threshold), rows.data_ptr(),
                                           offsets.data_ptr(), ctypes.addressof(count))
    if total < 0:
        raise ValueError("ao_amd pointgroup: bfs_cluster: a list lies outside ball_query_idxs or names a point outside [0, %d)" % n)
    return rows[:total].clone(), offsets[:count.value + 1].clone()


def _host_cluster(label, idx, start_len, min_points):
    """point_cluster, sizes, firsts from the host search (the reference's result also when a list was cut)"""
    dev = label.device
    rows, offsets = bfs_cluster(label.cpu(), idx.cpu(), start_len.cpu(), min_points)
    n = label.shape[0]
    point_cluster = torch.full((n,), -1, dtype=torch.int32)
    point_cluster[rows[:, 1].long()] = rows[:, 0]
    sizes = offsets[1:] - offsets[:-1]
    firsts = rows[offsets[:-1].long(), 1]
    return point_cluster.to(dev), sizes.to(dev), firsts.contiguous().to(dev)


def cluster(semantic_label, ball_query_idxs, start_len, min_points, capped=None):
    """The device form: (point_cluster (n) int32: the cluster of each point or -1, cluster_size (nCluster) int32,
    cluster_first (nCluster) int32: the first point of each cluster).  Without a cut list the clusters are the connected
    components of the edges whose ends carry the same label, numbered by their smallest member -- the order in which the
    reference's search seeds them.  `capped` (from ball_query; None: any len >= BALL_CAP counts as possibly cut): the lists
    are then a directed graph, and the reference's search runs on the host over one download of them."""
    _lib.require_cuda(semantic_label, ball_query_idxs, start_len)
    n = semantic_label.shape[0]
    dev = semantic_label.device
    if start_len.shape != (n, 2):
        raise ValueError("ao_amd pointgroup: %d labels for start_len %s" % (n, tuple(start_len.shape)))
    if n == 0:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return empty, empty.clone(), empty.clone()
    label = semantic_label.int().contiguous()
    idx, start_len = ball_query_idxs.int().contiguous(), start_len.int().contiguous()
    if capped is None:
        capped = bool((start_len[:, 1] >= BALL_CAP).any())
    if capped or not use_hip():
        return _host_cluster(label, idx, start_len, min_points)
    L = _lib.lib()
    point_cluster = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    firsts = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.ptv2_pg_cluster_workspace_bytes(n), dev)
    csr = _csr(idx, start_len)
    rc = L.pg_cluster_hip_launcher(n, label.data_ptr(), ctypes.addressof(csr), int(min_points), point_cluster.data_ptr(),
                                   sizes.data_ptr(), firsts.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _lib.stream_ptr())
    _lib.check(rc, "pg_cluster_hip_launcher")
    nc = int(count)
    return point_cluster, sizes[:nc], firsts[:nc]


# -------------------------------------------------------------------------------------------------------- proposals ----
def _proposals_torch(point_cluster, sizes, firsts, segment_pred, prob, propose_points):
    keep = (sizes > propose_points).nonzero().view(-1)
    masks = (point_cluster[None, :] == keep[:, None].int()).int()
    classes = segment_pred[firsts[keep].long()]
    scores = [prob[masks[j].bool(), classes[j]].mean() for j in range(keep.numel())]
    scores = torch.stack(scores) if scores else prob.new_zeros(0)
    return scores, masks, classes


def proposals(point_cluster, cluster_size, cluster_first, segment_pred, prob, propose_points, is_logit=False):
    """(scores (P) fp32, masks (P, N) int32, classes (P) int64) of the clusters with more than propose_points members, in
    cluster order: the class is segment_pred of the cluster's first point, the score the mean over the members of prob[:, class]
    (of softmax(prob) when is_logit).  The sum runs in a fixed order: the same input gives the same bits."""
    _lib.require_cuda(point_cluster, cluster_size, cluster_first, segment_pred, prob)
    n, nc = point_cluster.shape[0], cluster_size.shape[0]
    dev = point_cluster.device
    if prob.dim() != 2 or prob.shape[0] != n or segment_pred.shape != (n,) or not 1 <= prob.shape[1] <= MAX_CLASSES:
        raise ValueError("ao_amd pointgroup: prob %s and segment_pred %s for %d points" % (tuple(prob.shape), tuple(segment_pred.shape), n))
    prob = prob.float().contiguous()
    segment_pred = segment_pred.long().contiguous()
    if n == 0 or nc == 0:
        return (torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros((0, n), dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    point_cluster, cluster_size, cluster_first = (t.int().contiguous() for t in (point_cluster, cluster_size, cluster_first))
    if not use_hip():
        return _proposals_torch(point_cluster, cluster_size, cluster_first, segment_pred,
                                torch.softmax(prob, -1) if is_logit else prob, int(propose_points))
    L = _lib.lib()
    ws = _lib.workspace(L.ptv2_pg_proposals_workspace_bytes(n, nc), dev)
    of_cluster = torch.empty(nc, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.pg_proposals_count_hip_launcher(nc, cluster_size.data_ptr(), int(propose_points), of_cluster.data_ptr(), count.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "pg_proposals_count_hip_launcher")
    p = int(count)  # the read-back that sizes the masks: only the kept proposals get a row
    scores = torch.empty(p, dtype=torch.float32, device=dev)
    classes = torch.empty(p, dtype=torch.int64, device=dev)
    masks = torch.empty((p, n), dtype=torch.int32, device=dev)
    rc = L.pg_proposals_fill_hip_launcher(n, prob.shape[1], nc, p, point_cluster.data_ptr(), cluster_size.data_ptr(),
                                          cluster_first.data_ptr(), of_cluster.data_ptr(), segment_pred.data_ptr(), prob.data_ptr(),
                                          1 if is_logit else 0, _lib.ptr(classes) if p else 0, _lib.ptr(scores) if p else 0,
                                          _lib.ptr(masks) if p else 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "pg_proposals_fill_hip_launcher")
    return scores, masks, classes


# ------------------------------------------------------------------------------------------------------ offset loss ----
def bias_loss_torch(bias_pred, coord, instance_center, instance, ignore_index):
    """point_group_v1m1_base.py:80-92, statement for statement"""
    mask = (instance != ignore_index).float()
    bias_gt = instance_center - coord
    bias_dist = torch.sum(torch.abs(bias_pred - bias_gt), dim=-1)
    bias_l1_loss = torch.sum(bias_dist * mask) / (torch.sum(mask) + 1e-8)
    bias_pred_norm = bias_pred / (torch.norm(bias_pred, p=2, dim=1, keepdim=True) + 1e-8)
    bias_gt_norm = bias_gt / (torch.norm(bias_gt, p=2, dim=1, keepdim=True) + 1e-8)
    cosine_similarity = -(bias_pred_norm * bias_gt_norm).sum(-1)
    bias_cosine_loss = torch.sum(cosine_similarity * mask) / (torch.sum(mask) + 1e-8)
    return bias_l1_loss, bias_cosine_loss


class _BiasLoss(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, bias_pred, coord, instance_center, instance, ignore_index):
        bias_pred, coord, instance_center = bias_pred.contiguous(), coord.contiguous(), instance_center.contiguous()
        instance = instance.long().contiguous()
        n, dev = bias_pred.shape[0], bias_pred.device
        L = _lib.lib()
        out = torch.empty(3, dtype=torch.float32, device=dev)
        ws = _lib.workspace(L.ptv2_pg_bias_loss_workspace_bytes(n), dev)
        rc = L.pg_bias_loss_fwd_hip_launcher(n, bias_pred.data_ptr(), coord.data_ptr(), instance_center.data_ptr(),
                                             instance.data_ptr(), int(ignore_index), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr())
        _lib.check(rc, "pg_bias_loss_fwd_hip_launcher")
        ctx.save_for_backward(bias_pred, coord, instance_center, instance, out)
        ctx.ignore_index = int(ignore_index)
        return out[0], out[1]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_l1, g_cos):
        bias_pred, coord, instance_center, instance, out = ctx.saved_tensors
        g = torch.stack([g_l1.float().reshape(()), g_cos.float().reshape(())]).contiguous()
        d = torch.empty_like(bias_pred)
        rc = _lib.lib().pg_bias_loss_bwd_hip_launcher(bias_pred.shape[0], bias_pred.data_ptr(), coord.data_ptr(),
                                                      instance_center.data_ptr(), instance.data_ptr(), ctx.ignore_index,
                                                      out.data_ptr(), g.data_ptr(), d.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "pg_bias_loss_bwd_hip_launcher")
        return d, None, None, None, None


def bias_loss(bias_pred, coord, instance_center, instance, ignore_index=-1):
    """(bias_l1_loss, bias_cosine_loss) of bias_pred, coord, instance_center (n, 3) and instance (n), in fp32 (under autocast
    too): the mean over the rows with instance != ignore_index (divided by their number + 1e-8) of sum |pred - gt| and of
    -cos(pred, gt), gt = instance_center - coord, each vector normalised with + 1e-8."""
    _lib.require_cuda(bias_pred, coord, instance_center, instance)
    if bias_pred.dim() != 2 or bias_pred.shape[1] != 3 or coord.shape != bias_pred.shape or instance_center.shape != bias_pred.shape \
            or instance.shape != bias_pred.shape[:1]:
        raise ValueError("ao_amd pointgroup: bias_loss takes (n, 3), (n, 3), (n, 3), (n); got %s %s %s %s" % (
            tuple(bias_pred.shape), tuple(coord.shape), tuple(instance_center.shape), tuple(instance.shape)))
    if not use_hip() or bias_pred.shape[0] == 0:
        with torch.autocast("cuda", enabled=False):
            return bias_loss_torch(bias_pred.float(), coord.float(), instance_center.float(), instance, ignore_index)
    return _BiasLoss.apply(bias_pred, coord, instance_center, instance, ignore_index)
