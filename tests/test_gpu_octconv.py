"""GPU: OctFormer's dense octree convolutions and tables (ao_amd/csrc/oct_conv.hip) and the whole OctFormer-v1m1.

Exact: parent, child, up and down3 of octree_pyramid against the dictionary-built tables of tests/octconv_ref.py; two runs give
the same bits; shapes outside the supported set raise ValueError.

Against float64: y, g_x, g_w (and g_b with a bias) of every case of tests/octconv_cases.py, and logits and gradients of a small
OctFormer against the float64 run of its AO_AMD_OCTFORMER=torch path.  The bound is the rule of tests/test_gpu_st_ops.py:
e_kernel <= M[key] * max(e_eager, 2^-24) in relative L2, e_eager the fp32 run of the same reference on the same device.  M per
key: twice the worst ratio measured on the MI355X over all cases, rounded up to a power of two."""
import copy

import numpy as np
import pytest
import torch

from tests import octconv_cases as C
from tests import octconv_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
M = {"y": 4, "g_x": 8, "g_w": 4, "g_b": 4, "model": 4}
MODEL_KEYS = {"logits", "g_feat", "patch_embed.convs.0.conv.weights", "downsamples.0.conv.weights", "downsamples.0.conv.bias",
              "decoder.up_conv.1.deconv.weights", "seg_head.3.weight"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def check(tag, res, f64, f32, keys, bound=None):
    assert set(res) == keys and set(f64) == keys and set(f32) == keys
    bad = []
    for key in sorted(keys):
        assert torch.isfinite(res[key]).all(), key
        got, eager, m = _l2(res[key], f64[key]), _l2(f32[key], f64[key]), bound or M[key]
        print("octconv-ratio %-28s %-36s kernel %.3e  eager %.3e  ratio %.3f" % (tag, key, got, eager, got / max(eager, FLOOR)))
        if not got <= m * max(eager, FLOOR):
            bad.append((key, got, m * max(eager, FLOOR)))
    assert not bad, bad


def pyramid(name):
    from ao_amd.octformer import octree_pyramid

    t = C.tables(name)
    return octree_pyramid(_dev(t["xyz"]), _dev(t["batch"]), C.DEPTH, 2)


# ------------------------------------------------------------------------------------------------------- exact ----
@pytest.mark.parametrize("name", sorted(C.CLOUDS))
def test_tables_equal_the_dictionary(name):
    t, p = C.tables(name), pyramid(name)
    coarse, link = p.level(C.DEPTH - 1), p.link(C.DEPTH)
    assert np.array_equal(coarse.xyz.cpu().numpy(), t["pxyz"]) and np.array_equal(coarse.batch.cpu().numpy(), t["pbatch"])
    for key in ("parent", "child", "up", "down3"):
        assert np.array_equal(getattr(link, key).cpu().numpy(), t[key]), key
    up, down3 = link.up.cpu().numpy(), link.down3.cpu().numpy()
    j, k = np.nonzero(up >= 0)
    q, kk = np.nonzero(down3 >= 0)
    assert len(j) == len(q) and np.array_equal(down3[up[j, k], k], j) and np.array_equal(up[down3[q, kk], kk], q)


def run_layer(case, fn, dtype):
    t = C.layer_inputs(*case)
    x, w, b = (None if t[k] is None else _dev(t[k]).to(dtype).requires_grad_(True) for k in ("x", "weights", "bias"))
    y = fn(x, w, b, t)
    grads = torch.autograd.grad(y, [v for v in (x, w, b) if v is not None], _dev(t["g"]).to(dtype))
    return dict(zip(("y", "g_x", "g_w", "g_b"), (y.detach(),) + grads))


def ours(case):
    from ao_amd.octformer import octree_conv

    p = pyramid(case[4])
    table = p.level(C.DEPTH) if case[0] == "conv3" else p.link(C.DEPTH)
    return run_layer(case, lambda x, w, b, t: octree_conv(x, w, b, table, case[0]), torch.float32)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: "%s-%d-%d-%s" % (c[0], c[1], c[2], c[4]))
def test_octree_conv_against_float64(case):
    f64, f32 = (run_layer(case, lambda x, w, b, t: R.conv(x, w, b, _dev(t["tab"]), t["transpose"]), dt)
                for dt in (torch.float64, torch.float32))
    check("%s-%d-%d-%s" % (case[0], case[1], case[2], case[4]), ours(case), f64, f32, {"y", "g_x", "g_w"} | ({"g_b"} if case[3] else set()))


@pytest.mark.parametrize("case", [C.CASES[2], C.CASES[4], C.CASES[5]], ids=lambda c: c[0])
def test_two_runs_give_the_same_bits(case):
    a, b = ours(case), ours(case)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("cin,cout", [(10, 24), (24, 20), (24, 392)], ids=["cin-10", "cout-20", "cout-392"])
def test_outside_the_supported_shapes_raises(cin, cout):
    from ao_amd.octformer import octree_conv

    level = pyramid("tiny").level(C.DEPTH)
    with pytest.raises(ValueError):
        octree_conv(torch.zeros(level.n, cin, device="cuda"), torch.zeros(27, cin, cout, device="cuda"), None, level, "conv3")


# ------------------------------------------------------------------------------------------------- whole model ----
def model_run(model, data, g):
    feat = data["feat"].detach().to(next(model.parameters()).dtype).requires_grad_(True)
    logits = model(dict(data, feat=feat))
    model.zero_grad()
    (logits * g.to(logits.dtype)).sum().backward()
    params = dict(model.named_parameters())
    return dict({k: params[k].grad.clone() for k in MODEL_KEYS - {"logits", "g_feat"}}, logits=logits.detach(), g_feat=feat.grad)


def test_octformer_against_the_float64_run_of_its_eager_path(monkeypatch):
    """about 300 points in two clouds from the blob cloud of tests/octformer_cases.py: depth-9 cells become depth-7 leaves with
    several points each; the coarsest depth in use (4) keeps about 90 nodes per cloud for BatchNorm"""
    from ao_amd.octformer import OctFormer

    xyz, batch = C.OC.cloud((150, 150), seed=11)
    rng = np.random.default_rng(11)
    coord = ((xyz + 0.5) / 256.0 - 1.0) * 10.24   # cell (x, y, z) of depth 9 -> node (x, y, z) >> 2 of depth 7
    data = dict(coord=_dev(coord.astype(np.float32)), normal=None, feat=_dev(rng.standard_normal((300, 6)).astype(np.float32)),
                offset=_dev(np.cumsum(np.bincount(batch))))
    g = _dev(rng.standard_normal((300, 5)).astype(np.float32))
    torch.manual_seed(11)
    model = OctFormer(in_channels=6, num_classes=5, fpn_channels=24, channels=(32, 64), num_blocks=(1, 1), num_heads=(2, 4),
                      patch_size=8, dilation=2, stem_down=2, head_up=2, drop_path=0.0, octree_depth=7, octree_full_depth=2).cuda().train()
    res = model_run(copy.deepcopy(model), data, g)
    monkeypatch.setenv("AO_AMD_OCTFORMER", "torch")
    f32 = model_run(copy.deepcopy(model), data, g)
    f64 = model_run(copy.deepcopy(model).double(), data, g)
    assert res["logits"].shape == (300, 5)
    check("octformer", res, f64, f32, MODEL_KEYS, bound=M["model"])
