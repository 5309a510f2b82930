"""Float64 reference of the grouped-vector-attention stages and inputs on which no ReLU mask can flip.

Test infrastructure (plain torch, no project kernels).  The reference IS tests/gva_torch_ref.py::TorchImpl (pinned to the
oracle's literal _gva by tests/test_gva_host_logic.py and tests/test_gva_ref64_host.py) evaluated on float64 copies of the
inputs, extended by the grouped projection of ao_amd/csrc/gva_peb.hip

    out[n, 8 g + i] = out_v[n, 8 g + i] + sum_c' A[n, g, c'] Wp2[8 g + i, c'] + bp2[8 g + i] sw[n, g]

with every gradient from float64 autograd (ReLU'(0) = 0, as torch and the reference project have it).

Why special inputs.  A fp32 kernel and a float64 reference that disagree on the sign of ONE pre-activation differ by a whole
term, not by rounding, and a tolerance that absorbs that hides real defects.  build_inputs() makes both pre-activations exact:

    a . pos + b      coordinates in multiples of 2^-7 (so pos is), a in multiples of 2^-5 with |a| <= 8, b in multiples of 2^-6
    W1 * sc + sh     W1 in multiples of 2^-8 with |W1| <= 4, sc in multiples of 2^-4 in [0.5, 2.5], sh in multiples of 2^-6

Every product and every partial sum is then a multiple of 2^-12 of magnitude below 2^12, i.e. an integer of fewer than 24 bits
times 2^-12: exact in fp32 whatever the order of evaluation, with or without fused multiply-add.  A pre-activation is exactly 0
or at least 2^-12 away from 0, fp32 and float64 agree on every mask bit.  Exact zeros are planted on purpose (b[::5] = 0 with
the self slot's pos = 0; sh[::2] = 0 with W1[::3, 0, ::2] = 0; the duplicate points the coordinate rounding creates), so the
kink itself is exercised in every row.  check_inputs() asserts all of this for every case it is given: a case that does not
meet it is an error.  Everything else (kW, qW, M, cW, Ww2, bw2, v, Wp2, bp2, the upstream gradients) is generic random."""
import collections

import numpy as np
import torch

from tests import synth
from tests.gva_torch_ref import TorchImpl, _pos

Case = collections.namedtuple("Case", "name n c g k kind")

# keys of the float64 reference (and of the eager fp32 statement): the forward outputs ...
FWD_LOGITS = ("W1", "T1", "T2")
FWD_ATTN = ("w", "sw", "A", "out_v", "out")
# ... and every gradient
BWD_LOGITS = ("gkW", "gqW", "lga", "lgb", "gM", "gcW")           # (lga / lgb: grad a, b through the logits stage)
BWD_ATTN = ("gW1", "gsc", "gsh", "gWw2", "gbw2", "gv", "ga", "gb", "gWp2", "gbp2")
ALL_KEYS = FWD_LOGITS + FWD_ATTN + BWD_LOGITS + BWD_ATTN
ZERO_KEYS = ("gbw2",)  # the softmax is shift invariant: the true gradient is exactly 0, every implementation returns its noise

TILE_SHAPES = ((96, 12), (192, 24), (384, 48), (512, 64))   # k = 16: gva_fwd_tile.hip / gva_wgrad_tile.hip instances
BWD_TILE_SHAPES = ((96, 12), (192, 24), (384, 48))          # gva_bwd_tile.hip instances


def _cases():
    out = []

    def add(n, c, g, k=16, kind="std"):
        out.append(Case("%s-n%d-c%d-g%d-k%d" % (kind, n, c, g, k), n, c, g, k, kind))

    # the narrow full-resolution shape (point / flat / staged forms only), k = 16 and k = 8
    for n in (1, 5, 17, 127, 129, 3000):
        add(n, 48, 6)
    for n in (5, 17, 1000):
        add(n, 48, 6, k=8)
    # the tile shapes.  n on the dispatch edges of the code:
    #   1, 5, 17            a cloud shorter than K in every row; one ragged 4-, 8- and 16-point tile
    #   127, 128, 129       n % 16 = 15, 0, 1 (gva_fwd_tile.hip); the weight gradient's split n / 128 + 1 (wgrad.hip)
    #   1024, 1025          the 384-wide backward: 4-point tiles while (n + 3) / 4 <= 256, 8-point tiles beyond
    #   3072, 3080, 4096, 4097, 4501, 6144, 6152, 6500
    #                       bwd_tile_full_rounds (gva_bwd_tile.hip), slots = occupancy x CUs read at run time: whole rounds only
    #                       (plain 8-point launch) / a tail of at most half a round (mixed 8- / 4-point launch) / a longer
    #                       tail (plain), bracketed for 256 slots (3072 | 3080, 6144 | 6152) and 512 slots (4096 | 4097,
    #                       6144 | 6152)
    #   1074, 4501, 18905   the benchmark's level sizes
    small = (1, 5, 17, 127, 128, 129)
    for c, g in ((96, 12), (192, 24)):
        for n in small + (1074, 3072, 3080, 4096, 4097, 4501, 6144, 6152, 6500):
            add(n, c, g)
    add(18905, 96, 12)
    for n in small + (1024, 1025, 1074, 4501):
        add(n, 384, 48)
    for n in small + (1025, 1074):
        add(n, 512, 64)
    # softmax logits spread over about +-60 (forward only): a wrong max subtraction overflows or flushes with the hardware exp2
    for c, g in ((48, 6),) + TILE_SHAPES:
        add(700, c, g, kind="spread")
    # a hub: slot 1 of every row of the first segment points at ONE point (an inverse-table list about n long: gv, gkW)
    add(4501, 192, 24, kind="hub")
    return out


CASES = _cases()


def segment_sizes(n):
    return [n] if n < 40 else [n - 30, 9, 21]


def _dyadic(t, step, lo=None, hi=None):
    t = torch.round(t / step) * step
    return t if lo is None else t.clamp(lo, hi)


def build_inputs(case, knn, device="cpu"):
    """fp32 inputs of both stages for `case` on `device`; knn(k, coord, offset) -> idx int32 (n, k) with -1 placeholders."""
    n, c, g, k = case.n, case.c, case.g, case.k
    seed = 1000 + n + 7 * c + k
    sizes = segment_sizes(n)
    pts = np.concatenate([synth.room_cloud(max(m, 64), seed=seed + i)[:m] for i, m in enumerate(sizes)])
    coord = _dyadic(torch.from_numpy(pts), 2.0 ** -7).to(device)
    offset = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=device)
    idx = knn(k, coord, offset).contiguous().clone()
    if case.kind == "hub" and sizes[0] > k:
        idx[: sizes[0], 1] = sizes[0] // 2
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    t = dict(
        a=_dyadic(2.0 * r(c, 3), 2.0 ** -5, -8.0, 8.0), b=_dyadic(0.25 * r(c), 2.0 ** -6),
        W1=_dyadic(r(n, k, g), 2.0 ** -8, -4.0, 4.0), sc=_dyadic(0.5 + 2.0 * torch.rand(g, generator=gen), 2.0 ** -4, 0.5, 2.5),
        sh=_dyadic(0.3 * r(g), 2.0 ** -6),
        kW=r(n, g), qW=r(n, g), M=0.2 * r(c, g), cW=r(g),
        Ww2=r(g, g) / g ** 0.5, bw2=0.1 * r(g), v=r(n, c), Wp2=r(c, c) / c ** 0.5, bp2=0.1 * r(c),
        g_out=r(n, c), g_W1=r(n, k, g), g_T1=0.1 * r(g).double(), g_T2=0.01 * r(g).double())
    t["b"][::5] = 0.0
    t["sh"][::2] = 0.0
    t["W1"][::3, 0, ::2] = 0.0
    t = {key: val.to(device).contiguous() for key, val in t.items()}
    t.update(coord=coord.contiguous(), idx=idx, offset=offset, k=k)
    if case.kind == "spread":
        with torch.no_grad():
            z = torch.relu(t["W1"].double() * t["sc"].double() + t["sh"].double()) @ t["Ww2"].double().t()
            t["Ww2"] = (t["Ww2"] * (60.0 / float(z.abs().max()))).contiguous()
    return t


def preactivations(t, dtype):
    """(a . pos + b (n,k,c), W1 * sc + sh (n,k,g)) evaluated in `dtype`, the way TorchImpl does"""
    coord, a, b, W1, sc, sh = (t[key].to(dtype) for key in ("coord", "a", "b", "W1", "sc", "sh"))
    pos, _, _ = _pos(coord, t["idx"])
    return pos @ a.t() + b, W1 * sc + sh


def check_inputs(case, t):
    """The properties the float64 comparison rests on; returns counts for reports."""
    n, k = t["idx"].shape
    for key, step, hi in (("coord", 2.0 ** -7, 2.0 ** 5), ("a", 2.0 ** -5, 8.0), ("b", 2.0 ** -6, 8.0), ("W1", 2.0 ** -8, 4.0),
                          ("sc", 2.0 ** -4, 2.5), ("sh", 2.0 ** -6, 8.0)):
        val = t[key].double()
        assert torch.equal(torch.round(val / step) * step, val), (case.name, key, "not on its grid")
        assert float(val.abs().max()) <= hi, (case.name, key, float(val.abs().max()))
    assert float(t["sc"].min()) >= 0.5
    counts = {}
    for name, p32, p64 in zip(("pos", "w"), preactivations(t, torch.float32), preactivations(t, torch.float64)):
        assert torch.equal(p32.double(), p64), (case.name, name, "fp32 and float64 pre-activations differ")
        assert torch.equal(torch.round(p64 * 4096.0), p64 * 4096.0) and float(p64.abs().max()) < 4096.0, (case.name, name)
        assert torch.equal(p32 > 0, p64 > 0)
        zeros = int((p64 == 0).sum())
        assert zeros >= 1, (case.name, name, "no exact zero at the kink")
        counts["zeros_" + name] = zeros
    idx = t["idx"]
    assert int(idx.max()) < n and int(idx.min()) >= -1
    # slot 0 is the point itself or a duplicate of it: pos = 0 there, so b[::5] = 0 puts an exact zero into every row
    assert torch.equal(t["coord"][idx[:, 0].long()], t["coord"]), (case.name, "slot 0 is not at distance 0")
    counts["placeholders"] = int((idx < 0).sum())
    sizes = segment_sizes(case.n)
    if min(sizes) < k:
        assert counts["placeholders"] >= 1, (case.name, "a cloud shorter than K must leave -1 slots")
    if case.kind == "hub":
        assert int((idx == sizes[0] // 2).sum()) >= sizes[0]
    return counts


def project(A, Wp2, bp2, sw, out_v):
    n, g, c = A.shape
    i = c // g
    return out_v + torch.einsum("ngc,gic->ngi", A, Wp2.view(g, i, c)).reshape(n, c) + (sw.unsqueeze(-1) * bp2.view(1, g, i)).reshape(n, c)


def softmax_weights(t, dtype):
    """w (n,k,g): the softmax of TorchImpl.aggregate on its own (the statement returns only its sums)"""
    W1, sc, sh, Ww2, bw2 = (t[key].to(dtype) for key in ("W1", "sc", "sh", "Ww2", "bw2"))
    mask = (t["idx"] >= 0).to(dtype)
    return torch.softmax(torch.relu(W1 * sc + sh) @ Ww2.t() + bw2, dim=1) * mask.unsqueeze(-1)


def statement(t, dtype, backward=True):
    """TorchImpl (+ the grouped projection) on `dtype` copies of the inputs: dict over ALL_KEYS (forward keys only without
    `backward`).  dtype = float64 is the reference; dtype = float32 is the eager statement whose own distance from the
    reference scales the bound of the kernels."""
    coord, idx = t["coord"].to(dtype), t["idx"]
    leaf = lambda key: t[key].detach().to(dtype).clone().requires_grad_(backward)
    res = {}
    L = [leaf(key) for key in ("kW", "qW", "a", "b", "M", "cW")]
    W1, T1, T2 = TorchImpl.logits(*L, coord, idx)
    res.update(W1=W1, T1=T1, T2=T2)
    S = [leaf(key) for key in ("W1", "sc", "sh", "Ww2", "bw2", "v", "a", "b")]
    Wp2, bp2 = leaf("Wp2"), leaf("bp2")
    out_v, A, sw = TorchImpl.aggregate(*S, coord, idx)
    out = project(A, Wp2, bp2, sw, out_v)
    res.update(w=softmax_weights(t, dtype), sw=sw, A=A, out_v=out_v, out=out)
    if backward:
        grads = torch.autograd.grad([W1, T1, T2], L, [t["g_W1"].to(dtype), t["g_T1"], t["g_T2"]])
        res.update(zip(BWD_LOGITS, grads))
        grads = torch.autograd.grad(out, S + [Wp2, bp2], t["g_out"].to(dtype))
        res.update(zip(BWD_ATTN, grads))
    return {key: val.detach() for key, val in res.items()}


def errors(got, ref):
    """(relative L2, largest element error over the largest reference element) of `got` against the float64 `ref`"""
    got, ref = got.double(), ref.double()
    diff = got - ref
    return (float(diff.norm() / ref.norm().clamp_min(1e-300)), float(diff.abs().max() / ref.abs().max().clamp_min(1e-300)))
