"""CPU: the host side of Point Transformer V1 (ao_amd/ptv1, include/ptv2_ptv1_hip.h) and the fixtures' own consistency."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import ptv1_cases as PC
from tests import ptv1_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("PointTransformer-Seg26", "PointTransformer-Seg38", "PointTransformer-Seg50")
# gradients of biases in front of a BatchNorm or the softmax: the true value is zero and both sides hold rounding noise, so
# they are compared to TOL of the norm of their weight's gradient (the sums they are the residue of)
ZERO_BIASES = ("linear_p.0.bias", "linear_w.2.bias", "linear_w.5.bias", "linear_q.bias", "linear_k.bias")
TOL = 1e-6


@pytest.fixture
def deterministic():
    """torch's CPU index_put(accumulate=True) adds with atomics from several threads (two runs of one model differ by 1e-6 in
    the gradient of feat); the fixtures were generated with the deterministic form"""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(before)


def _rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("name", PC.GOLDEN_LAYER_CASES)
def test_ref_layer_reproduces_the_reference_layer(name, golden, deterministic):
    from oracle import pointops_ref as P

    z = golden("ptv1_layer.npz")
    c = PC.case(name)
    t = {k: torch.from_numpy(v) for k, v in PC.layer_inputs(c).items()}
    layer = R.Layer(c.c, c.ns)
    layer.load_state_dict(PC.layer_state(layer, c), strict=True)
    layer.train()
    idx, _ = P.knn_query(c.ns, t["coord"], torch.tensor(np.cumsum(c.clouds), dtype=torch.int32))
    assert torch.equal(idx, t["idx"]), "the case's brute-force table is the oracle's"
    x = t["x_q"].clone().requires_grad_(True)
    y = layer(t["coord"], x, idx)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(y, [x] + list(params.values()), t["g_out"])
    res = {"out": y.detach(), "g_x": grads[0]}
    res.update({"g:" + k: g for k, g in zip(params, grads[1:])})
    assert {name + "/" + k for k in res} == {k for k in z.files if k.startswith(name + "/")}
    for key, got in res.items():
        ref = torch.from_numpy(z[name + "/" + key])
        if key.endswith(ZERO_BIASES) and float(ref.norm()) < 1e-3:
            scale = float(torch.from_numpy(z[name + "/" + key[:-4] + "weight"]).norm())
            assert float((got - ref).norm()) <= TOL * scale, key
        else:
            assert _rel(got, ref) <= TOL, (key, _rel(got, ref))


def test_ref_model_reproduces_the_reference_fp32_run(golden, deterministic):
    z, ze = golden("ptv1_model.npz"), golden("ptv1_model_eval.npz")
    batch = {k: torch.from_numpy(v) for k, v in PC.model_batch().items()}
    model = R.Seg()
    state = PC.fill_state(PC.shapes_of(model), PC.MODEL_SEED)
    model.load_state_dict(state, strict=True)
    model.eval()
    with torch.no_grad():
        assert _rel(model(batch), torch.from_numpy(ze["f32/eval_logits"])) <= TOL
    model.train()
    feat = batch["feat"].clone().requires_grad_(True)
    logits = model(dict(batch, feat=feat))
    loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
    loss.backward()
    got = {"logits": logits.detach(), "loss": loss.detach(), "g_feat": feat.grad}
    after = model.state_dict()
    got.update({k[4:]: after[k[6:]] for k in z.files if k.startswith("f32/b:")})
    assert {"f32/" + k for k in got} == {k for k in z.files if k.startswith("f32/")}
    for key, value in got.items():
        assert _rel(value, torch.from_numpy(z["f32/" + key])) <= TOL, key
    for key in z.files:
        if key.startswith("f64/b:") and key.endswith("num_batches_tracked"):
            assert int(after[key[6:]]) == int(z[key])
    # the level offsets the fixture was designed for: level 5 has -1 slots and every cloud keeps at least 3 points
    sizes = [c for c, _ in PC.MODEL_CLOUDS]
    for _ in range(4):
        sizes = [s // 4 for s in sizes]
    assert sizes == [8, 5] and min(sizes) >= 3 and min(sizes) < 16


def test_manifest_and_strict_loading():
    from ao_amd import ptv1

    with open(os.path.join(GOLDEN, "ptv1_manifest.json")) as f:
        manifest = json.load(f)
    classes = dict(zip(NAMES, (ptv1.PointTransformerSeg26, ptv1.PointTransformerSeg38, ptv1.PointTransformerSeg50)))
    assert set(manifest) == set(NAMES)
    for name in NAMES:
        model = classes[name](in_channels=6, num_classes=13)
        have = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert have == manifest[name], name
        assert list(have) == list(manifest[name]), "the reference's key order"
        ref = R.Seg(name)
        assert {k: list(v.shape) for k, v in ref.state_dict().items()} == manifest[name]
        state = PC.fill_state(PC.shapes_of(ref), 3)
        ref.load_state_dict(state, strict=True)
        model.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(model.state_dict(), strict=True)
        for key, value in model.state_dict().items():
            assert torch.equal(value, state[key]), key
    assert len(manifest[NAMES[0]]) == 564 and len(manifest[NAMES[2]]) == 932
    count = lambda m: sum(p.numel() for p in m.parameters())  # noqa: E731
    assert count(classes[NAMES[0]]()) == 4854145 and count(classes[NAMES[2]]()) == 7767729


def test_registry_files_the_three_names():
    from ao_amd import ptv1
    from ao_amd.ptv2 import registry

    class Fake:
        def __init__(self):
            self.modules = {}

        def register_module(self, module=None, name=None, force=False):
            self.modules[name] = module

    fake = Fake()
    done = registry.register(MODELS=fake)
    assert done == ["PT-v2m2", "DefaultSegmentor", "DefaultSegmentorSAM_Image"]
    assert fake.modules["PointTransformer-Seg26"] is ptv1.PointTransformerSeg26
    assert fake.modules["PointTransformer-Seg38"] is ptv1.PointTransformerSeg38
    assert fake.modules["PointTransformer-Seg50"] is ptv1.PointTransformerSeg50
    model = fake.modules["PointTransformer-Seg50"](in_channels=6, num_classes=13)
    assert model.cls[3].out_features == 13


def test_header_is_exported_and_bound():
    from ao_amd import _abi, _lib

    L = _lib.lib()
    names = {"ptv2_ptv1_abi_version", "ptv2_ptv1_struct_bytes", "ptv1_attention_workspace_bytes", "ptv1_attention_saved_bytes",
             "ptv1_attention_forward_hip_launcher", "ptv1_attention_backward_hip_launcher"}
    assert set(_abi.ptv1_signatures) == names
    with open(_abi.PTV1_HEADER) as f:
        text = f.read()
    for name, (restype, argtypes) in _abi.ptv1_signatures.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        params = text.split(name + "(", 1)[1].split(")", 1)[0]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert L.ptv2_ptv1_abi_version() == _lib.EXPECTED_PTV1_ABI == 1
    for which, name in enumerate(("ptv1_params", "ptv1_norms", "ptv1_grads")):
        assert L.ptv2_ptv1_struct_bytes(which) == ctypes.sizeof(_abi.ptv1_structs[name])
    assert L.ptv2_ptv1_struct_bytes(3) == -1
    # the other headers are as they were
    assert _lib.EXPECTED_ABI == 11 and L.ptv2_abi_version() == 11


def test_memory_rule():
    """workspace + saved: at most half of one (n, ns, C) fp32 tensor plus sixteen (n, C) tensors, at the five S3DIS level shapes"""
    from ao_amd import _lib

    L = _lib.lib()
    for n, ns, c in PC.LEVEL_SHAPES:
        ws, saved = L.ptv1_attention_workspace_bytes(n, ns, c), L.ptv1_attention_saved_bytes(n, ns, c)
        assert ws > 0 and saved >= 2 * 4 * n * ns * (c // 8)
        assert ws + saved <= 4 * n * ns * c // 2 + 16 * 4 * n * c, (n, ns, c, ws, saved)
    for bad in ((-1, 16, 64), (100, 0, 64), (100, 17, 64), (100, 16, 48), (100, 16, 1024)):
        assert L.ptv1_attention_workspace_bytes(*bad) == -1 and L.ptv1_attention_saved_bytes(*bad) == -1


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_no_cpu_fallback(path, monkeypatch):
    from ao_amd import ptv1

    monkeypatch.setenv("AO_AMD_PTV1", path)
    c = PC.case("c32")
    t = {k: torch.from_numpy(v) for k, v in PC.layer_inputs(c).items()}
    layer = ptv1.PointTransformerLayer(32, 32, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ptv1.vector_attention(t["x_q"], t["x_k"], t["x_v"], t["coord"], t["idx"], layer.linear_p, layer.linear_w)
    model = ptv1.PointTransformerSeg26(in_channels=6, num_classes=13)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model({k: torch.from_numpy(v) for k, v in PC.model_batch().items()})
