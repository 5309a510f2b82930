"""Point Transformer V1 (PointTransformer-Seg26 / 38 / 50) on the MI355X.

Reference: pointcept/models/point_transformer/point_transformer_seg.py.  Same constructor keywords, same state-dict keys and
shapes (`load_state_dict(strict=True)` works in both directions), same results; the execution differs:

  * the vector-attention layer between the q / k / v Linears and bn2 is one autograd node on ao_amd/csrc/ptv1.hip
    (ao_amd/ptv1/attention.py) and never forms an (n, ns, C) tensor;
  * everything else is composed from what the package has: RowLinear / RowBatchNorm1d / lin_bn_relu / bn_residual_relu
    (ao_amd/ptv2/layers.py) and pointops' farthest_point_sampling, knn_query, grouping and interpolation kernels;
  * one self-kNN table and one inverse table per level and forward, shared by every Bottleneck of that level in the encoder
    and the decoder (the reference recomputes the same table in every Bottleneck: 18 times per forward for Seg50);
  * `new_offset` of a TransitionDown comes from one host read of `offset` (the FPS wrapper synchronises anyway);
  * TransitionUp's head form takes the per-cloud mean as a product with a (clouds, points) matrix: no per-cloud python
    slicing of device scalars, and a backward without atomics;
  * gradients that the reference scatters with atomics (grouping, interpolation) are fixed-order gathers over inverse tables,
    so two identical steps give the same bits.
"""
import torch
import torch.nn as nn

from .. import _lib, pointops
from ..pointops.interpolation import _InterpolateRows, interpolation_index_weight
from ..ptv2 import gva
from ..ptv2.layers import RowBatchNorm1d, RowLinear, bn_residual_relu, lin_bn_relu
from .attention import vector_attention


class LayerNorm1d(nn.BatchNorm1d):
    """The reference's name (point_transformer/utils.py:7-14): a BatchNorm1d over the rows of an (n, ns, c) tensor."""

    def forward(self, input):
        return super().forward(input.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


class _GroupRows(torch.autograd.Function):
    """input (n, c), idx (m, ns) -> (m, ns, c), zeros where idx == -1 (pointops.grouping's kernel).  The gradient is a
    fixed-order gather, not pointops.grouping's atomic scatter: the table is read as (m * ns, 1) -- one slot per row, weight
    `ones` -- and summed over its inverse by the interpolation gather.  inverse_table sizes its lists by the table's row count,
    so this needs n <= m * ns (a TransitionDown keeps a quarter of the points with 16 slots each: m * ns is about 4 n); a
    table that is too short raises instead of taking the atomic path without notice."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, input, idx, ones):
        input = input.contiguous()
        m, ns = idx.shape
        n, c = input.shape
        out = torch.empty((m, ns, c), dtype=torch.float32, device=input.device)
        rc = _lib.lib().grouping_forward_hip_launcher(m, ns, c, input.data_ptr(), idx.data_ptr(), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "grouping_forward_hip_launcher")
        ctx.n = n
        if ctx.needs_input_grad[0]:
            if n > m * ns:
                raise RuntimeError("ao_amd ptv1: a (%d, %d) neighbour table is too short for the gather gradient of %d rows"
                                   % (m, ns, n))
            ctx.save_for_backward(ones, *gva.inverse_table(idx.view(-1, 1)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        ones, inv_ptr, inv_rows = ctx.saved_tensors
        g = g.contiguous()
        c = g.shape[2]
        gin = torch.empty((ctx.n, c), dtype=torch.float32, device=g.device)
        rc = _lib.lib().interpolation_backward_gather_hip_launcher(ctx.n, c, 1, g.data_ptr(), inv_ptr.data_ptr(),
                                                                   inv_rows.data_ptr(), ones.data_ptr(), gin.data_ptr(),
                                                                   _lib.stream_ptr())
        _lib.check(rc, "interpolation_backward_gather_hip_launcher")
        return gin, None, None


def _linear(cin, cout, bias=True):
    """RowLinear (the split-K weight gradient) where both widths are multiples of 4, nn.Linear for 3 + C, 6 and 13"""
    return (RowLinear if cin % 4 == 0 and cout % 4 == 0 else nn.Linear)(cin, cout, bias=bias)


class PointTransformerLayer(nn.Module):
    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16):
        super().__init__()
        self.mid_planes = mid_planes = out_planes // 1
        self.out_planes = out_planes
        self.share_planes = share_planes
        self.nsample = nsample
        if share_planes != 8:
            raise ValueError("ao_amd ptv1: share_planes is 8 (include/ptv2_ptv1_hip.h: PTV1_SHARE)")
        self.linear_q = RowLinear(in_planes, mid_planes)
        self.linear_k = RowLinear(in_planes, mid_planes)
        self.linear_v = RowLinear(in_planes, out_planes)
        self.linear_p = nn.Sequential(nn.Linear(3, 3), LayerNorm1d(3), nn.ReLU(inplace=True), nn.Linear(3, out_planes))
        self.linear_w = nn.Sequential(
            LayerNorm1d(mid_planes), nn.ReLU(inplace=True), nn.Linear(mid_planes, out_planes // share_planes),
            LayerNorm1d(out_planes // share_planes), nn.ReLU(inplace=True),
            nn.Linear(out_planes // share_planes, out_planes // share_planes))
        self.softmax = nn.Softmax(dim=1)

    def forward(self, pxo, idx=None, stats=None):
        """pxo = [coord (n, 3), feat (n, c), offset (b)]; idx: the level's self-kNN table (n, nsample) int32 when the caller has
        it (computed here otherwise, as the reference does)."""
        p, x, o = pxo
        if idx is None:
            idx = pointops.knn_query(self.nsample, p, o)[0]
        x_q, x_k, x_v = self.linear_q(x), self.linear_k(x), self.linear_v(x)
        return vector_attention(x_q, x_k, x_v, p, idx, self.linear_p, self.linear_w, stats)


class TransitionDown(nn.Module):
    def __init__(self, in_planes, out_planes, stride=1, nsample=16):
        super().__init__()
        self.stride, self.nsample = stride, nsample
        if stride != 1:
            self.linear = _linear(3 + in_planes, out_planes, bias=False)
            self.pool = nn.MaxPool1d(nsample)
        else:
            self.linear = _linear(in_planes, out_planes, bias=False)
        self.bn = RowBatchNorm1d(out_planes)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, pxo):
        p, x, o = pxo
        if self.stride == 1:
            return [p, lin_bn_relu(self.linear, self.bn, x), o]
        ends = [int(v) for v in o.tolist()]  # the one host read
        n_o, count, prev = [], 0, 0
        for e in ends:
            count += (e - prev) // self.stride
            prev = e
            n_o.append(count)
        n_o = torch.tensor(n_o, dtype=torch.int32, device=o.device)
        sel = pointops.farthest_point_sampling(p, o, n_o)
        n_p = p[sel.long(), :].contiguous()
        idx = pointops.knn_query(self.nsample, p, o, n_p, n_o)[0].contiguous()
        m = n_p.shape[0]
        mask = torch.sign(idx + 1).to(p.dtype).unsqueeze(-1)
        ones = torch.ones(idx.numel(), dtype=torch.float32, device=idx.device)  # the gather gradient's slot weights
        rel = (_GroupRows.apply(p, idx, ones) - n_p.unsqueeze(1)) * mask
        rows = torch.cat((rel, _GroupRows.apply(x.contiguous(), idx, ones)), -1).reshape(m * self.nsample, -1)
        y = lin_bn_relu(self.linear, self.bn, rows)  # the BatchNorm runs over the m * nsample rows
        return [n_p, y.reshape(m, self.nsample, -1).max(dim=1).values, n_o]


class TransitionUp(nn.Module):
    def __init__(self, in_planes, out_planes=None):
        super().__init__()
        if out_planes is None:
            self.linear1 = nn.Sequential(RowLinear(2 * in_planes, in_planes), RowBatchNorm1d(in_planes), nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(RowLinear(in_planes, in_planes), nn.ReLU(inplace=True))
        else:
            self.linear1 = nn.Sequential(RowLinear(out_planes, out_planes), RowBatchNorm1d(out_planes), nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(RowLinear(in_planes, out_planes), RowBatchNorm1d(out_planes), nn.ReLU(inplace=True))

    def forward(self, pxo1, pxo2=None):
        if pxo2 is None:
            _, x, o = pxo1
            # member (b, n): 1 where the point belongs to the cloud; the head level has a few hundred points
            ends = o.long()
            at = torch.arange(x.shape[0], device=x.device)
            member = ((at[None, :] < ends[:, None]) & (at[None, :] >= (ends - torch.diff(ends, prepend=ends.new_zeros(1)))[:, None]))
            member = member.to(x.dtype)
            mean = (member / member.sum(1, keepdim=True)) @ x
            x = torch.cat((x, member.t() @ self.linear2(mean)), 1)
            return lin_bn_relu(self.linear1[0], self.linear1[1], x)
        p1, x1, o1 = pxo1
        p2, x2, o2 = pxo2
        idx, weight = interpolation_index_weight(p2, p1, o2, o1)
        if torch.is_grad_enabled():
            # _InterpolateRows' backward looks for the inverse table on the index tensor and gathers in a fixed order when it
            # finds one (it scatters with atomics otherwise): inverse_table leaves it there
            gva.inverse_table(idx)
        up = _InterpolateRows.apply(lin_bn_relu(self.linear2[0], self.linear2[1], x2), idx, weight)
        return lin_bn_relu(self.linear1[0], self.linear1[1], x1) + up


class Bottleneck(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, share_planes=8, nsample=16):
        super().__init__()
        self.linear1 = RowLinear(in_planes, planes, bias=False)
        self.bn1 = RowBatchNorm1d(planes)
        self.transformer = PointTransformerLayer(planes, planes, share_planes, nsample)
        self.bn2 = RowBatchNorm1d(planes)
        self.linear3 = RowLinear(planes, planes * self.expansion, bias=False)
        self.bn3 = RowBatchNorm1d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, pxo, idx=None):
        p, x, o = pxo
        identity = x
        x = lin_bn_relu(self.linear1, self.bn1, x)
        x = self.bn2(self.transformer([p, x, o], idx), relu=True)
        x = bn_residual_relu(self.bn3, self.linear3(x), identity)
        return [p, x, o]


class PointTransformerSeg(nn.Module):
    def __init__(self, block, blocks, in_channels=6, num_classes=13):
        super().__init__()
        self.in_channels = in_channels
        self.in_planes, planes = in_channels, [32, 64, 128, 256, 512]
        stride, self.nsample = [1, 4, 4, 4, 4], [8, 16, 16, 16, 16]
        for i in range(5):
            down = TransitionDown(self.in_planes, planes[i] * block.expansion, stride[i], self.nsample[i])
            setattr(self, "enc%d" % (i + 1), self._stage(block, down, planes[i], blocks[i], self.nsample[i]))
        for i in range(4, -1, -1):
            up = TransitionUp(self.in_planes, None if i == 4 else planes[i] * block.expansion)  # level 5: the head form
            setattr(self, "dec%d" % (i + 1), self._stage(block, up, planes[i], 1, self.nsample[i]))
        self.cls = nn.Sequential(RowLinear(planes[0], planes[0]), RowBatchNorm1d(planes[0]), nn.ReLU(inplace=True),
                                 _linear(planes[0], num_classes))

    def _stage(self, block, first, planes, blocks, nsample):
        """nn.Sequential(first, block x blocks): index 0 is the transition, the Bottlenecks follow (the reference's key layout)"""
        self.in_planes = planes * block.expansion
        return nn.Sequential(first, *[block(self.in_planes, self.in_planes, 8, nsample=nsample) for _ in range(blocks)])

    def forward(self, data_dict):
        p = data_dict["coord"].float().contiguous()
        x = data_dict["feat"].contiguous()
        o = data_dict["offset"].int().contiguous()
        _lib.require_cuda(p, x, o)
        levels = []  # (p, x, o, idx) per level
        for i in range(5):
            enc = getattr(self, "enc%d" % (i + 1))
            p, x, o = enc[0]([p, x, o])
            idx = pointops.knn_query(self.nsample[i], p, o)[0].contiguous()  # THE self-kNN of the level
            if torch.is_grad_enabled():
                gva.inverse_table(idx)  # cached on the table: every layer's backward of the level finds it there
            for blk in list(enc)[1:]:
                p, x, o = blk([p, x, o], idx)
            levels.append([p, x, o, idx])
        for i in range(4, -1, -1):
            dec = getattr(self, "dec%d" % (i + 1))
            p, x, o, idx = levels[i]
            x = dec[0]([p, x, o]) if i == 4 else dec[0]([p, x, o], levels[i + 1][:3])
            for blk in list(dec)[1:]:
                p, x, o = blk([p, x, o], idx)
            levels[i][1] = x
        x = lin_bn_relu(self.cls[0], self.cls[1], levels[0][1])
        return self.cls[3](x)


class PointTransformerSeg26(PointTransformerSeg):
    def __init__(self, **kwargs):
        super().__init__(Bottleneck, [1, 1, 1, 1, 1], **kwargs)


class PointTransformerSeg38(PointTransformerSeg):
    def __init__(self, **kwargs):
        super().__init__(Bottleneck, [1, 2, 2, 2, 2], **kwargs)


class PointTransformerSeg50(PointTransformerSeg):
    def __init__(self, **kwargs):
        super().__init__(Bottleneck, [1, 2, 3, 5, 2], **kwargs)
