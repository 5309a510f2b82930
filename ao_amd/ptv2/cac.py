"""CAC-v1m1: the context-aware classifier segmentor of the reference
(pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py), on a PT-v2m2 backbone.

Constructor, defaults, module tree and state_dict keys are the reference's (`seg_head`, `proj.{0,2}`, `apd_proj.{0,2}`,
`feat_proj_layer.{0,1,3}` with the BatchNorm buffers); `seg_head` and `feat_proj_layer` run on the N-row layers
(RowLinear / RowBatchNorm1d), the K-row MLPs `proj` / `apd_proj` stay plain torch.  The returns of the three modes follow
`forward` (:200-270): training -> dict(loss, seg_loss, pre_loss, pre_self_loss, kl_loss); eval with `segment` -> the loss of
the backbone head's logits and the REFINED logits as `seg_logits`; eval without -> `seg_logits` only.

The reference's heads loop in python over every present class (twice, after two `target.unique()` host synchronisations)
and over the scenes with device-tensor slice bounds.  Here the soft prototypes, the class means, the cosine logits and the
distillation loss are ao_amd/csrc/cac.hip: a fixed number of launches whatever the class count, no host synchronisation.
Scene bounds come from `input_dict["offset_host"]` when present (no synchronisation), else from ONE `offset.tolist()`.

Kept quirks: the ignore label of the CAC heads is -1 whatever the criteria's `ignore_index` (:78-80, :162-180);
`feat_proj_layer` runs once per scene inside the refine branch, in scene order, and then once on the whole batch
(training-mode BatchNorm: per-scene batch statistics, B + 1 running-statistics updates per step); the distillation target
of an ignored row puts its one-hot half on class 0 (its entropy weight is 0).

Deviation: under autocast the CAC kernels take fp32 inputs (`custom_fwd(cast_inputs=torch.float32)`) where the reference
forms the prototype and cosine products in half precision.

The HIP path covers CUDA inputs with K <= 256 classes and backbone_out_channels C % 4 == 0, 4 <= C <= 64.  Anything else
(CPU tensors, other shapes), and every input under AO_AMD_CAC=torch (an A/B switch), takes a vectorised eager formulation of
the same contract."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers import RowBatchNorm1d, RowLinear
from .model import PointTransformerV2
from .segmentor import _parse_criteria, cross_entropy

MAX_CLASSES, MAX_CHANNELS = 256, 64
PROTO_EPS, MEAN_EPS = 1e-7, 1e-4


def native_ok(x, num_classes):
    """Whether the HIP kernels take (N, C) rows `x` with `num_classes` classes."""
    c = x.shape[1] if x.dim() == 2 else 0
    return (x.is_cuda and os.environ.get("AO_AMD_CAC", "hip") != "torch" and x.shape[0] > 0
            and 1 <= num_classes <= MAX_CLASSES and c % 4 == 0 and 4 <= c <= MAX_CHANNELS)


# ------------------------------------------------------------------------------------------------------------ HIP path
class _WeightedSum(torch.autograd.Function):
    """mode 0: soft prototypes per scene (z (B,K), protos (B,K,C)); mode 1: class means over the batch (counts (1,K),
    means (1,K,C))."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, logits, label, offset, k, max_rows, thr, eps, mode):
        from .. import _lib

        x = x.contiguous()
        logits = logits.contiguous() if logits is not None else None
        n, c = x.shape
        b = offset.numel()
        sets = b if mode == 0 else 1
        dev = x.device
        z = torch.empty((sets, k), dtype=torch.float32, device=dev)
        out = torch.empty((sets, k, c), dtype=torch.float32, device=dev)
        L = _lib.lib()
        ws = _lib.workspace(L.cac_workspace_bytes(b, max_rows, n, k, c), dev)
        rc = L.cac_weighted_sum_forward_hip_launcher(mode, n, b, max_rows, k, c, x.data_ptr(), _lib.ptr(logits), _lib.ptr(label),
                                                     offset.data_ptr(), float(thr), float(eps), z.data_ptr(), out.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "cac_weighted_sum_forward_hip_launcher")
        ctx.save_for_backward(x, logits, label, offset, z, out)
        ctx.args = (k, max_rows, float(thr), float(eps), mode)
        ctx.mark_non_differentiable(z)
        return z, out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gz, gout):
        from .. import _lib

        x, logits, label, offset, z, out = ctx.saved_tensors
        k, max_rows, thr, eps, mode = ctx.args
        n, c = x.shape
        gx = torch.empty_like(x)
        glogits = torch.empty_like(logits) if mode == 0 and ctx.needs_input_grad[1] else None
        gout = gout.contiguous().float()
        rc = _lib.lib().cac_weighted_sum_backward_hip_launcher(
            mode, n, offset.numel(), max_rows, k, c, x.data_ptr(), _lib.ptr(logits), _lib.ptr(label), offset.data_ptr(), thr,
            eps, z.data_ptr(), out.data_ptr(), gout.data_ptr(), gx.data_ptr(), _lib.ptr(glogits), _lib.stream_ptr())
        _lib.check(rc, "cac_weighted_sum_backward_hip_launcher")
        return gx, glogits, None, None, None, None, None, None, None


class _Cosine(torch.autograd.Function):
    """scale * <x_n / max(|x_n|, 1e-12), q_k / max(|q_k|, 1e-12)>; q (B,K,C) one set per scene, or (K,C) shared."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, q, offset, max_rows, scale):
        from .. import _lib

        x, q = x.contiguous(), q.contiguous()
        n, c = x.shape
        k = q.shape[-2]
        per_scene = int(q.dim() == 3)
        out = torch.empty((n, k), dtype=torch.float32, device=x.device)
        rc = _lib.lib().cac_cosine_forward_hip_launcher(n, offset.numel(), max_rows, k, c, x.data_ptr(), q.data_ptr(), per_scene,
                                                        offset.data_ptr(), float(scale), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "cac_cosine_forward_hip_launcher")
        ctx.save_for_backward(x, q, offset)
        ctx.args = (max_rows, float(scale), per_scene)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        from .. import _lib

        x, q, offset = ctx.saved_tensors
        max_rows, scale, per_scene = ctx.args
        n, c = x.shape
        k = q.shape[-2]
        b = offset.numel()
        g = g.contiguous().float()
        gx, gq = torch.empty_like(x), torch.empty_like(q)
        L = _lib.lib()
        ws = _lib.workspace(L.cac_workspace_bytes(b, max_rows, n, k, c), x.device)
        rc = L.cac_cosine_backward_hip_launcher(n, b, max_rows, k, c, x.data_ptr(), q.data_ptr(), per_scene, offset.data_ptr(),
                                                scale, g.data_ptr(), gx.data_ptr(), gq.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr())
        _lib.check(rc, "cac_cosine_backward_hip_launcher")
        return gx, gq, None, None, None


class _Distill(torch.autograd.Function):
    """get_distill_loss(pred, soft, target) (smoothness 0.5, eps 0); the gradient goes to `pred` only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, pred, soft, label):
        from .. import _lib

        pred, soft = pred.contiguous(), soft.detach().contiguous()
        n, k = pred.shape
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(k, dtype=torch.float32, device=dev)
        L = _lib.lib()
        ws = _lib.workspace(L.cac_workspace_bytes(1, 1, n, k, 4), dev)
        rc = L.cac_distill_forward_hip_launcher(n, k, pred.data_ptr(), soft.data_ptr(), label.data_ptr(), loss.data_ptr(),
                                                coef.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "cac_distill_forward_hip_launcher")
        ctx.save_for_backward(pred, soft, label, coef)
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        from .. import _lib

        pred, soft, label, coef = ctx.saved_tensors
        n, k = pred.shape
        g = g.reshape(1).contiguous().float()
        gp = torch.empty_like(pred)
        rc = _lib.lib().cac_distill_backward_hip_launcher(n, k, pred.data_ptr(), soft.data_ptr(), label.data_ptr(),
                                                          coef.data_ptr(), g.data_ptr(), gp.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "cac_distill_backward_hip_launcher")
        return gp, None, None


# ---------------------------------------------------------------------------------------------------------- eager path
def _soft_protos_torch(x, logits, bounds, thr):
    """(B, K, C) soft prototypes, the reference's per-scene formula (:128-137)."""
    out, lo = [], 0
    for hi in bounds:
        p = F.softmax(logits[lo:hi].float(), 1).permute(1, 0)
        if thr > 0:
            p = p * (p.max(0)[0] >= thr).float().unsqueeze(0)
        out.append((p / (p.sum(-1).unsqueeze(-1) + PROTO_EPS)) @ x[lo:hi].float())
        lo = hi
    return torch.stack(out)


def _class_means_torch(x, label, k):
    """(means (K, C), present (K,)) of the rows with a label in [0, K)."""
    # a one-hot product, not index_add: on the device that adds with float atomics, and two identical steps then differ in the
    # last place (a label outside [0, K) matches no column)
    hot = (label.unsqueeze(1) == torch.arange(k, device=label.device).unsqueeze(0)).float()
    cnt = hot.sum(0)
    sums = hot.t() @ x.float()
    return sums / (cnt + MEAN_EPS)[:, None], cnt > 0


def _cosine_torch(x, q, bounds, scale):
    xn = F.normalize(x.float(), 2, 1)
    if q.dim() == 2:
        return xn @ F.normalize(q.float(), 2, 1).t() * scale
    out, lo = [], 0
    for s, hi in enumerate(bounds):
        out.append(xn[lo:hi] @ F.normalize(q[s].float(), 2, 1).t() * scale)
        lo = hi
    return torch.cat(out, 0)


def _distill_torch(pred, soft, target):
    """get_distill_loss (:152-198), vectorised over the classes."""
    pred, soft = pred.float(), soft.detach().float()
    n, k = soft.shape
    ignore = target == -1
    hot = torch.where(ignore, torch.zeros_like(target), target)
    sm = F.softmax(soft, 1)
    onehot = torch.zeros((n, k), dtype=torch.float32, device=pred.device).scatter_(1, hot.unsqueeze(1), 1)
    loss = (-F.log_softmax(pred, 1) * (0.5 * sm + 0.5 * onehot)).sum(1)
    valid = (~ignore).float()
    ent = -(sm * torch.log(sm + 1e-4)).sum(1) * valid
    num = torch.zeros(k, dtype=torch.float32, device=pred.device).index_add(0, hot, loss * ent)
    den = torch.zeros(k, dtype=torch.float32, device=pred.device).index_add(0, hot, ent)
    cnt = torch.zeros(k, dtype=torch.float32, device=pred.device).index_add(0, hot, valid)
    present = cnt > 0
    per = torch.where(present, num / (den + 1e-4), torch.zeros_like(num))
    return per.sum() / (present.float().sum() + 1e-4)


# ------------------------------------------------------------------------------------------------------------ segmentor
def distill_loss(pred, soft, target):
    """get_distill_loss(pred, soft.detach(), target) with smoothness 0.5, eps 0: HIP for CUDA inputs with K <= 256."""
    if pred.is_cuda and pred.dim() == 2 and os.environ.get("AO_AMD_CAC", "hip") != "torch" and 1 <= pred.shape[1] <= MAX_CLASSES \
            and pred.shape[0] > 0:
        return _Distill.apply(pred, soft.detach(), target.contiguous())
    return _distill_torch(pred, soft, target)


def _build_backbone(backbone):
    if isinstance(backbone, nn.Module):
        return backbone
    cfg = dict(backbone)
    kind = cfg.pop("type", "PT-v2m2")
    if kind != "PT-v2m2":
        raise NotImplementedError("CAC-v1m1: backbone type %r is not supported here; the backbone must be PT-v2m2 "
                                  "(or an nn.Module)" % (kind,))
    return PointTransformerV2(**cfg)


class CACSegmentor(nn.Module):
    """Registry name "CAC-v1m1" (reference :15)."""

    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None, cos_temp=15, main_weight=1,
                 pre_weight=1, pre_self_weight=1, kl_weight=1, conf_thresh=0, detach_pre_logits=False):
        super().__init__()
        self.num_classes = num_classes
        self.cos_temp = cos_temp
        self.main_weight = main_weight
        self.pre_weight = pre_weight
        self.pre_self_weight = pre_self_weight
        self.kl_weight = kl_weight
        self.conf_thresh = conf_thresh
        self.detach_pre_logits = detach_pre_logits
        self.backbone = _build_backbone(backbone)
        c = backbone_out_channels
        self.seg_head = RowLinear(c, num_classes)
        self.proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.apd_proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.feat_proj_layer = nn.Sequential(RowLinear(c, c, bias=False), RowBatchNorm1d(c), nn.ReLU(inplace=True),
                                             RowLinear(c, c))
        self._criteria = _parse_criteria(criteria, -1)

    @property
    def _ddp_params_and_buffers_to_ignore(self):
        from .model import parallel_ddp_ignore

        return parallel_ddp_ignore(self, "backbone.") if isinstance(self.backbone, PointTransformerV2) else []

    def loss(self, seg_logits, segment):
        """the criteria summed in config order (DefaultSegmentor.loss)"""
        total = None
        for weight, ignore, lovasz in self._criteria:
            if lovasz is not None:
                term = lovasz(seg_logits, segment)
            else:
                term = cross_entropy(seg_logits, segment, ignore)
                term = term if weight == 1.0 else term * weight
            total = term if total is None else total + term
        return total

    @staticmethod
    def scene_bounds(input_dict):
        """row ends of the scenes: `offset_host` (no synchronisation) or ONE offset.tolist()"""
        bounds = input_dict.get("offset_host")
        if bounds is None:
            bounds = input_dict["offset"].tolist()
        return [int(v) for v in bounds]

    def _native(self, feat):
        return native_ok(feat, self.num_classes)

    def _feat_proj_per_scene(self, feat, bounds):
        if not self.training:  # (BatchNorm on its running statistics is row-local: one call is the per-scene result)
            return self.feat_proj_layer(feat)
        out, lo = [], 0
        for hi in bounds:
            out.append(self.feat_proj_layer(feat[lo:hi]))
            lo = hi
        return torch.cat(out, 0) if len(out) > 1 else out[0]

    def refine_logits(self, feat, seg_logits, bounds, offset):
        """post_refine_proto_batch (:97-150) * cos_temp"""
        proto = self.seg_head.weight
        pred = seg_logits.detach() if self.detach_pre_logits else seg_logits
        k, c = proto.shape
        b = len(bounds)
        native = self._native(feat)
        if native:
            offset32 = offset.to(device=feat.device, dtype=torch.int32)
            max_rows = max(hi - lo for lo, hi in zip([0] + bounds[:-1], bounds))
            _, protos = _WeightedSum.apply(feat, pred, None, offset32, k, max_rows, float(self.conf_thresh), PROTO_EPS, 0)
        else:
            protos = _soft_protos_torch(feat, pred, bounds, self.conf_thresh)
        protos = self.proj(torch.cat([protos, proto.unsqueeze(0).expand(b, k, c).to(protos.dtype)], -1))
        x = self._feat_proj_per_scene(feat, bounds)
        if native:
            return _Cosine.apply(x, protos, offset32, max_rows, float(self.cos_temp))
        return _cosine_torch(x, protos, bounds, self.cos_temp)

    def adaptive_logits(self, feat, target, bounds, offset):
        """get_adaptive_perspective (:72-95) * cos_temp"""
        proto = self.seg_head.weight
        k, c = proto.shape
        native = self._native(feat)
        if native:
            offset32 = offset.to(device=feat.device, dtype=torch.int32)
            max_rows = max(hi - lo for lo, hi in zip([0] + bounds[:-1], bounds))
            cnt, means = _WeightedSum.apply(feat, None, target.contiguous(), offset32, k, max_rows, 0.0, MEAN_EPS, 1)
            means, present = means[0], cnt[0] > 0
        else:
            means, present = _class_means_torch(feat, target, k)
        new_proto = torch.where(present.unsqueeze(1), means.to(proto.dtype), proto.detach())
        new_proto = self.apd_proj(torch.cat([new_proto, proto], -1))
        x = self.feat_proj_layer(feat)
        if native:
            return _Cosine.apply(x, new_proto, offset32, max_rows, float(self.cos_temp))
        return _cosine_torch(x, new_proto, bounds, self.cos_temp)

    def forward(self, data_dict):
        offset = data_dict["offset"]
        feat = self.backbone(data_dict)
        seg_logits = self.seg_head(feat)
        bounds = self.scene_bounds(data_dict)
        refine = self.refine_logits(feat, seg_logits, bounds, offset)
        if self.training:
            target = data_dict["segment"]
            cac_pred = self.adaptive_logits(feat, target, bounds, offset)
            seg_loss = self.loss(refine, target) * self.main_weight
            pre_loss = self.loss(cac_pred, target) * self.pre_weight
            pre_self_loss = self.loss(seg_logits, target) * self.pre_self_weight
            kl_loss = distill_loss(refine, cac_pred.detach(), target) * self.kl_weight
            loss = seg_loss + pre_loss + pre_self_loss + kl_loss
            return dict(loss=loss, seg_loss=seg_loss, pre_loss=pre_loss, pre_self_loss=pre_self_loss, kl_loss=kl_loss)
        if "segment" in data_dict:
            return dict(loss=self.loss(seg_logits, data_dict["segment"]), seg_logits=refine)
        return dict(seg_logits=refine)
