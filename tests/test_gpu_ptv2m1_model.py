"""GPU: PT-v2m1 (GroupedLinear + position multiplier) against fixtures captured from the reference nn.Module
(tests/golden/ptv2m1.npz, written by tests/golden/make_golden_ptv2m1.py), in both modes: the default (the multiplier logits
stage of ao_amd/csrc/gva_mul.hip inside the staged composition) and AO_AMD_GVA=unfused (the literal op sequence).

Tolerances are those of the PT-v2m2 fixture tests (tests/test_gpu_model.py): module output and logits
1e-4, loss 2e-5, parameter gradients in relative L2 (2e-2 through the model), running buffers rtol 1e-4 / atol 1e-6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ptv2m1_cases as C
from tests.test_oracle_model import assert_grad_close

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(params=["fused", "unfused"])
def gva_mode(request, monkeypatch):
    monkeypatch.setenv("AO_AMD_GVA", request.param)
    return request.param


def _attention(c, g, pe_multiplier=True):
    from ao_amd.ptv2.model import GroupedVectorAttention, use_grouped_linear

    return use_grouped_linear(GroupedVectorAttention(c, g, pe_multiplier=pe_multiplier, pe_bias=True))


def _count_stage_calls(monkeypatch):
    from ao_amd.ptv2 import gva

    calls = []
    real = gva._HipImpl.logits_mul
    monkeypatch.setattr(gva._HipImpl, "logits_mul", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    return calls


@pytest.mark.parametrize("c,g", C.SHAPES)
def test_attention_module_matches_reference_module(golden, monkeypatch, gva_mode, c, g):
    from ao_amd.ptv2 import gva

    gold = golden("ptv2m1.npz")
    tag = "attn%d_" % c
    attn = _attention(c, g)
    st = C.init_state({k: v.shape for k, v in attn.state_dict().items()}, C.MODULE_SEED + c)
    assert C.state_digest(st) == str(gold[tag + "digest"])
    attn = attn.cuda()
    coord, offset, feat0, gout = C.module_inputs(c)
    idx = dev(gold[tag + "idx"])
    assert int((idx < 0).sum()) >= idx.shape[0]
    calls = _count_stage_calls(monkeypatch)
    for mode in ("train", "eval"):
        attn.load_state_dict(st, strict=True)
        attn.train(mode == "train")
        feat = feat0.cuda().requires_grad_(True)
        out = attn(feat, coord.cuda(), idx)
        np.testing.assert_allclose(out.detach().cpu().numpy(), gold[tag + "out_" + mode], rtol=1e-4, atol=1e-4)
        if mode == "train":
            names = [k[len(tag) + 2:] for k in gold.files if k.startswith(tag + "g_")]
            assert "weight_encoding.0.weight" in names and "linear_p_multiplier.0.weight" in names
            params = dict(attn.named_parameters())
            grads = torch.autograd.grad(out, [feat] + [params[n] for n in names], gout.cuda())
            np.testing.assert_allclose(grads[0].cpu().numpy(), gold[tag + "gfeat"], rtol=1e-3, atol=1e-4)
            for n, gr in zip(names, grads[1:]):
                assert_grad_close(gr.cpu().numpy(), gold[tag + "g_" + n], n)
            sd = attn.state_dict()
            bufs = [k for k in gold.files if k.startswith(tag + "buf_")]
            assert len(bufs) == 6
            for k in bufs:
                np.testing.assert_allclose(sd[k[len(tag) + 4:]].cpu().numpy(), gold[k], rtol=1e-4, atol=1e-6, err_msg=k)
    fused_here = gva_mode == "fused" and gva.mul_supported(c, g, idx.shape[0], idx.shape[1])
    assert len(calls) == (2 if fused_here else 0)  # the default path IS the new stage, the switch IS the literal one


def _model():
    from ao_amd.ptv2 import PointTransformerV2M1

    model = PointTransformerV2M1(**C.MODEL_CFG)
    st = C.init_state({k: v.shape for k, v in model.state_dict().items()}, C.MODEL_SEED)
    return model.cuda(), st


def test_model_matches_reference_module(golden, monkeypatch, gva_mode):
    gold = golden("ptv2m1.npz")
    model, st = _model()
    assert C.state_digest(st) == str(gold["model_digest"])
    coord, offset, feat, label = (t.cuda() for t in C.model_inputs())
    data = dict(coord=coord, feat=feat, offset=offset)
    calls = _count_stage_calls(monkeypatch)
    for mode in ("train", "eval"):
        model.load_state_dict(st, strict=True)
        model.train(mode == "train")
        logits = model(data)
        np.testing.assert_allclose(logits.detach().cpu().numpy(), gold["model_logits_" + mode], rtol=0, atol=1e-4)
        loss = F.cross_entropy(logits, label, ignore_index=-1)
        assert abs(float(loss) - float(gold["model_loss_" + mode])) < 2e-5
        if mode == "train":
            names = [n for n, _ in model.named_parameters()]
            assert all("model_grad_" + n in gold.files for n in names)
            for n, gr in zip(names, torch.autograd.grad(loss, list(model.parameters()))):
                ref = gold["model_grad_" + n]
                if n.endswith(".0.bias") and float(np.abs(ref).max()) < 1e-6:  # a bias in front of a BatchNorm: true gradient 0
                    assert float(gr.abs().max()) < 1e-4, n
                    continue
                assert_grad_close(gr.cpu().numpy(), ref, n, rel_l2=2e-2, frac_max=5e-2)
            sd = model.state_dict()
            for k in gold.files:
                if k.startswith("model_buf_"):
                    np.testing.assert_allclose(sd[k[len("model_buf_"):]].cpu().numpy(), gold[k], rtol=1e-4, atol=1e-6, err_msg=k)
    assert (len(calls) > 0) == (gva_mode == "fused")


@pytest.mark.parametrize("pe_multiplier", [True, False])
def test_never_enters_the_native_runtimes(pe_multiplier):
    from ao_amd.ptv2 import PointTransformerV2M1, block, native_model

    model = PointTransformerV2M1(**dict(C.MODEL_CFG, pe_multiplier=pe_multiplier)).cuda()
    coord, offset, feat, _ = (t.cuda() for t in C.model_inputs())
    for mode in (True, False):
        model.train(mode)
        assert not native_model.supported(model, feat)
        blk = model.patch_embed.blocks.blocks[0]
        idx = torch.zeros((feat.shape[0], 8), dtype=torch.int32, device="cuda")
        assert not block.supported(blk, torch.zeros(feat.shape[0], 48, device="cuda"), idx)
    with torch.no_grad():
        assert bool(torch.isfinite(model(dict(coord=coord, feat=feat, offset=offset))).all())


def test_grouped_linear_without_multiplier_matches_the_literal_float64_statement():
    """GroupedLinear with pe_multiplier=False runs the literal op sequence on the HIP gather kernel: against the same module
    in float64 on the CPU (its grouping answered by the oracle's plain-torch one)."""
    import copy
    import types

    from ao_amd import pointops
    from ao_amd.ptv2 import model as model_py
    from oracle import pointops_ref as P

    c, g = 48, 6
    attn = _attention(c, g, pe_multiplier=False)
    attn.load_state_dict(C.init_state({k: v.shape for k, v in attn.state_dict().items()}, 7), strict=True)
    ref_mod = copy.deepcopy(attn).double().train()
    coord, offset, feat0, gout = C.module_inputs(c)
    idx = pointops.knn_query(16, coord.cuda(), offset.cuda())[0]
    real = model_py.pointops
    model_py.pointops = types.SimpleNamespace(grouping=P.grouping)
    try:
        f64 = feat0.double().requires_grad_(True)
        ref = ref_mod(f64, coord.double(), idx.cpu())
        (rg,) = torch.autograd.grad(ref, f64, gout.double())
    finally:
        model_py.pointops = real
    attn = attn.cuda().train()
    feat = feat0.cuda().requires_grad_(True)
    out = attn(feat, coord.cuda(), idx)
    (gr,) = torch.autograd.grad(out, feat, gout.cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gr.cpu().numpy(), rg.numpy(), rtol=1e-3, atol=1e-4)


def test_eval_forward_uses_the_running_statistics():
    model, st = _model()
    coord, offset, feat, _ = (t.cuda() for t in C.model_inputs())
    data = dict(coord=coord, feat=feat, offset=offset)
    model.load_state_dict(st, strict=True)
    model.eval()
    with torch.no_grad():
        y0 = model(data)
        key = "patch_embed.blocks.blocks.0.attn.linear_p_multiplier.1.norm.running_mean"
        st2 = dict(st)
        st2[key] = st[key] + 0.5
        model.load_state_dict(st2, strict=True)
        y1 = model(data)
    assert bool(torch.equal(model.state_dict()[key].cpu(), st2[key]))  # eval mode left the buffers alone
    assert float((y1 - y0).abs().max()) > 1e-4


def test_two_training_steps_through_the_segmentor():
    from ao_amd.ptv2 import DefaultSegmentor, PointTransformerV2M1
    from ao_amd.ptv2.optim import FlatAdamW

    torch.manual_seed(0)
    seg = DefaultSegmentor(dict(C.MODEL_CFG, type="PT-v2m1")).cuda().train()
    assert isinstance(seg.backbone, PointTransformerV2M1)
    coord, offset, feat, label = (t.cuda() for t in C.model_inputs())
    data = dict(coord=coord, feat=feat, offset=offset, segment=label)
    opt = FlatAdamW(seg.parameters(), lr=0.006, weight_decay=0.05)
    losses = []
    for _ in range(3):  # (two steps, the loss after each)
        loss = seg(data)["loss"]
        losses.append(float(loss))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
