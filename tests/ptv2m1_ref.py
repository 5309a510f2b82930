"""Plain-torch statement of the multiplier logits stage of PT-v2m1 (ao_amd/csrc/gva_mul.hip, include/ptv2_v2m1_hip.h).

Test infrastructure (plain torch, no project kernels), in the manner of tests/gva_torch_ref.py: `logits_mul` is the stage,
`TorchImplM1` puts it beside the PT-v2m2 stages so that the host logic of ao_amd/ptv2/gva.py can be driven on the CPU, and
`statement` evaluates the stage and every gradient by autograd in a given precision (float64: the reference; float32: the
eager statement whose own distance from float64 scales the bound of the kernels)."""
import torch

from tests.gva_torch_ref import TorchImpl, _pos

FWD = ("W1", "T1", "T2")
BWD = ("g_key", "g_query", "g_w", "g_a_m", "g_b_m", "g_Wm2", "g_bm2", "g_a", "g_b", "g_M", "g_cW")
INPUTS = ("key", "query", "w", "a_m", "b_m", "Wm2", "bm2", "a", "b", "M", "cW")  # the order of logits_mul, BWD alike
ALL_KEYS = FWD + BWD


def logits_mul(key, query, w, a_m, b_m, Wm2, bm2, a, b, M, cW, coord, idx):
    """W1 (n,k,g), T1 (g), T2 (g) float64: the formulas of include/ptv2_v2m1_hip.h, one op per line"""
    pos, mask, safe = _pos(coord, idx)
    n, k = idx.shape
    c, g = M.shape
    Pm = torch.relu(pos @ a_m.t() + b_m)
    pem = Pm @ Wm2.t() + bm2
    P = torch.relu(pos @ a.t() + b)
    rel = key[safe] * mask.unsqueeze(-1) - query.unsqueeze(1)
    W1 = (rel * pem * w).view(n, k, g, c // g).sum(-1) + P @ M + cW
    W1d = W1.double()
    return W1, W1d.sum((0, 1)), (W1d * W1d).sum((0, 1))


class TorchImplM1(TorchImpl):
    logits_mul = staticmethod(logits_mul)


def statement(t, dtype, backward=True):
    """dict over ALL_KEYS (FWD only without `backward`) of logits_mul on `dtype` copies of the inputs t"""
    leaves = [t[key].detach().to(dtype).clone().requires_grad_(backward) for key in INPUTS]
    W1, T1, T2 = logits_mul(*leaves, t["coord"].to(dtype), t["idx"])
    res = dict(W1=W1, T1=T1, T2=T2)
    if backward:
        res.update(zip(BWD, torch.autograd.grad([W1, T1, T2], leaves, [t["g_W1"].to(dtype), t["g_T1"], t["g_T2"]])))
    return {key: val.detach() for key, val in res.items()}


def literal_m(weight_w, Wp2, bp2, groups):
    """(M (C,G), cW (G)) as ao_amd/ptv2/gva.py forms them from GroupedLinear.weight[0], linear_p_bias[3]"""
    c = weight_w.shape[0]
    i = c // groups
    return (Wp2 * weight_w.unsqueeze(1)).view(groups, i, c).sum(1).t().contiguous(), (weight_w * bp2).view(groups, i).sum(1)
