"""GPU: a BasicLayer(48, depth 2, 6 heads, window 5, quant 4, XYZ_RGB_NORM) of ao_amd.swin3d -- one plain and one shifted block --
on the two-clouds case of tests/swin3d_cases.py: the output, the input gradient and every parameter gradient of the default path
against the float64 run of the same module under AO_AMD_SWIN3D=torch, under the rule of tests/test_gpu_swin3d_ops.py (e_eager:
the fp32 run under the switch).  The state-dict manifest is written out from swin3d_layers.py of the reference."""
import copy

import numpy as np
import pytest
import torch

from tests import swin3d_cases as SC

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
# M: 2 x the worst e_kernel / max(e_eager, 2^-24), as a power of two; "g_param" is shared by the
# parameter gradients
M = {"out": 2, "g_feats": 4, "g_param": 4}

ATTN = [("attn.%s_%s_table" % (role, key), (3, rows, 6, 8)) for key, rows in (("xyz", 40), ("rgb", 32), ("norm", 32))
        for role in ("query", "key", "value")]
BLOCK = ([("norm1.weight", (48,)), ("norm1.bias", (48,))] + ATTN +
         [("attn.qkv.weight", (144, 48)), ("attn.qkv.bias", (144,)), ("attn.proj.weight", (48, 48)), ("attn.proj.bias", (48,)),
          ("norm2.weight", (48,)), ("norm2.bias", (48,)), ("mlp.fc1.weight", (192, 48)), ("mlp.fc1.bias", (192,)),
          ("mlp.fc2.weight", (48, 192)), ("mlp.fc2.bias", (48,))])
MANIFEST = [("blocks.%d.%s" % (i, k), shape) for i in range(2) for k, shape in BLOCK]


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def layer_of():
    from ao_amd.swin3d import BasicLayer

    torch.manual_seed(0)
    layer = BasicLayer(48, 2, 6, 5, 4, drop_path=0.0, cRSE="XYZ_RGB_NORM").cuda().train()
    with torch.no_grad():   # tables that matter, LayerNorm affine terms away from (1, 0)
        for k, p in layer.named_parameters():
            if k.endswith("_table"):
                p.normal_(std=0.5)
            elif "norm" in k:
                p.uniform_(0.5, 1.5) if k.endswith("weight") else p.normal_(std=0.2)
    return layer


def test_state_dict_manifest():
    assert [(k, tuple(v.shape)) for k, v in layer_of().state_dict().items()] == MANIFEST


def test_downsample_is_the_follow_up():
    from ao_amd.swin3d import BasicLayer

    with pytest.raises(NotImplementedError):
        BasicLayer(48, 2, 6, 5, 4, downsample=torch.nn.Identity)


def test_layer_against_float64(monkeypatch):
    layer = layer_of()
    t = SC.cloud("two-clouds")
    grid, batch, local, colors = (torch.from_numpy(t[k]).cuda() for k in ("grid_coord", "batch", "local_xyz", "colors"))
    rng = np.random.default_rng(5)
    feats, g_out = (torch.from_numpy(rng.standard_normal((len(grid), 48)).astype(np.float32)).cuda() for _ in range(2))
    names = [k for k, _ in layer.named_parameters()]

    def run(module, dtype):
        x = feats.to(dtype).requires_grad_(True)
        out = module(x, grid, batch, local, colors)
        grads = torch.autograd.grad(out, [x] + [p for _, p in module.named_parameters()], g_out.to(dtype))
        return dict(zip(["out", "g_feats"] + ["g_" + k for k in names], (out.detach(),) + grads))

    res = run(layer, torch.float32)
    monkeypatch.setenv("AO_AMD_SWIN3D", "torch")
    f64, f32 = run(copy.deepcopy(layer).double(), torch.float64), run(layer, torch.float32)
    assert set(res) == set(f64) == set(f32) == {"out", "g_feats"} | {"g_" + k for k in names} and len(names) == len(MANIFEST)
    bad = []
    for key in sorted(res):
        got, eager, m = _l2(res[key], f64[key]), _l2(f32[key], f64[key]), M.get(key, M["g_param"])
        print("swin-layer-ratio %-40s kernel %.3e  eager %.3e  ratio %.3f" % (key, got, eager, got / max(eager, FLOOR)))
        if not got <= m * max(eager, FLOOR):
            bad.append((key, got, m * max(eager, FLOOR)))
    assert not bad, bad
