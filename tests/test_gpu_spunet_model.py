"""GPU: BasicBlock and the whole SpUNet-v1m1 (ao_amd/spunet/model.py) against the float64 run of tests/spunet_ref.py on the
device, on both paths (HIP and AO_AMD_SPUNET=torch).

The bound is the M-rule of tests/test_gpu_spunet_conv.py: |ours - f64| <= M[output] * max(|eager fp32 - f64|, 2^-24 |f64|) in L2
(for the logits and a block's output also in the largest element), the eager fp32 run being tests/spunet_ref.py in fp32 on the
same device and inputs.  M per output class: twice the worst ratio measured on the MI355X over both paths, rounded up to a power
of two and not below 1.  A float64 gradient whose norm is below 1e-12 is its own rounding noise (there is
none in this model: no bias sits in front of a BatchNorm).  num_batches_tracked is compared exactly.

The seeds keep every ReLU pre-activation at least spunet_cases.MARGIN from its kink in float64 (asserted here on the device run;
tests/golden/make_golden_spunet.py --seeds finds them on the CPU)."""
import numpy as np
import pytest
import torch

from tests import spunet_cases as SC
from tests import spunet_ref as R

pytestmark = pytest.mark.gpu

# M per output class
M_BLOCK = {"out": 8, "g_in": 8, "grad": 8, "buffer": 2}
M_MODEL = {"logits": 8, "loss": 1, "grad": 8, "buffer": 4}
FLOOR = 2.0 ** -24
_REF = {}


def _bound(M, kind, name, got, f64, f32, bad, peak=False):
    err = float((got.double() - f64).norm())
    allowed = M[kind] * max(float((f32.double() - f64).norm()), FLOOR * float(f64.norm()))
    print("spunet-model-ratio %-7s %-44s err %.3e allowed %.3e ratio-to-eager %.3f" % (kind, name, err, allowed, err / (allowed / M[kind])))
    if not err <= allowed:
        bad.append((name, err, allowed))
    if peak:
        perr = float((got.double() - f64).abs().max())
        pallowed = M[kind] * max(float((f32.double() - f64).abs().max()), FLOOR * float(f64.abs().max()))
        print("spunet-model-ratio %-7s %-44s err %.3e allowed %.3e ratio-to-eager %.3f" % (kind, name + " (peak)", perr, pallowed, perr / (pallowed / M[kind])))
        if not perr <= pallowed:
            bad.append((name + " peak", perr, pallowed))


def _compare(M, got, f64, f32, peaks):
    assert set(got) == set(f64) == set(f32)
    bad = []
    for key in sorted(got):
        if key.endswith("num_batches_tracked"):
            assert int(got[key]) == int(f64[key]), key
            continue
        assert torch.isfinite(got[key]).all(), key
        kind = key if key in M else "buffer" if key.startswith("b:") else "grad"
        _bound(M, kind, key, got[key], f64[key], f32[key], bad, peak=key in peaks)
    assert not bad, bad


def _buffers(module):
    return {"b:" + k: v.detach().clone() for k, v in module.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}


# ------------------------------------------------------------------------------------------------------------ the block ----
def _block_geometry(form):
    from ao_amd import spunet

    coord, offset, x, g = SC.block_inputs(form)
    ref = R.tables_to(R.build_tables(coord, offset, levels=1), "cuda")
    ours = spunet.build_tables(torch.from_numpy(coord).cuda(), torch.from_numpy(offset).cuda())
    return ref, ours, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()


def _block_state(form):
    cin, cout = SC.BLOCK_WIDTHS[form]
    return SC.fill_state(SC.shapes_of(R.Block(cin, cout)), 300 + SC.BLOCK_SEEDS[form])


def _block_ref(form, training, dtype, tables, x0, g0):
    block = R.Block(*SC.BLOCK_WIDTHS[form])
    block.load_state_dict(_block_state(form), strict=True)
    block = block.to(device="cuda", dtype=dtype).train(training)
    x = x0.to(dtype).requires_grad_(training)
    R.Margin.reset()
    out = block(x, tables, 0)
    res = {"out": out.detach()}
    if training:
        grads = torch.autograd.grad(out, [x] + list(block.parameters()), g0.to(dtype))
        res.update(zip(["g_in"] + ["g:" + k for k, _ in block.named_parameters()], grads))
    res.update(_buffers(block))
    return res, R.Margin.value


def _block_op(form, training, tables, x0, g0):
    from ao_amd import spunet
    from ao_amd.spunet.model import _norm

    block = spunet.BasicBlock(*SC.BLOCK_WIDTHS[form], norm_fn=_norm, indice_key="subm0")
    block.load_state_dict(_block_state(form), strict=True)
    block = block.cuda().train(training)
    x = x0.clone().requires_grad_(training)
    out = block(spunet.SparseTensor(x, tables, 0)).features
    res = {"out": out.detach()}
    if training:
        grads = torch.autograd.grad(out, [x] + list(block.parameters()), g0)
        res.update(zip(["g_in"] + ["g:" + k for k, _ in block.named_parameters()], grads))
    res.update(_buffers(block))
    return res


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("form", ["same", "proj"])
def test_block_against_float64(form, training, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", path)
    key = ("block", form, training)
    if key not in _REF:
        ref, ours, x, g = _block_geometry(form)
        (f64, margin), (f32, _) = _block_ref(form, training, torch.float64, ref, x, g), _block_ref(form, training, torch.float32, ref, x, g)
        _REF[key] = (ours, x, g, f64, f32, margin)
    ours, x, g, f64, f32, margin = _REF[key]
    assert margin > SC.MARGIN, "the case's inputs put a ReLU pre-activation %.2e from its kink" % margin
    got = _block_op(form, training, ours, x, g)
    n_params = {"same": 6, "proj": 9}[form]
    assert len(got) == (1 + (1 + n_params if training else 0) + {"same": 6, "proj": 9}[form])
    print("spunet-case block", form, "train" if training else "eval", path)
    _compare(M_BLOCK, got, f64, f32, {"out"})


# ------------------------------------------------------------------------------------------------------------ the model ----
def _batch():
    return {k: torch.from_numpy(v).cuda() for k, v in SC.model_batch().items()}


def _state(classes=13):
    return SC.fill_state(SC.shapes_of(R.SpUNet(6, classes)), SC.MODEL_SEED)


def _model(classes=13):
    from ao_amd import spunet

    model = spunet.SpUNetBase(6, classes)
    model.load_state_dict(_state(classes), strict=True)
    return model.cuda()


def _step(model, batch):
    model.train()
    model.zero_grad(set_to_none=True)
    logits = model(batch)
    loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
    loss.backward()
    return logits.detach(), loss.detach()


def _collect(model, logits, loss):
    res = {"logits": logits, "loss": loss}
    res.update({"g:" + k: p.grad for k, p in model.named_parameters()})
    res.update(_buffers(model))
    return res


def _device_reference():
    if "model" not in _REF:
        batch = _batch()
        tables = R.tables_to(R.build_tables(batch["discrete_coord"].cpu().numpy(), batch["offset"].cpu().numpy()), "cuda")
        runs = []
        for dtype in (torch.float64, torch.float32):
            model = R.SpUNet(6, 13)
            model.load_state_dict(_state(), strict=True)
            model = model.to(device="cuda", dtype=dtype).train()
            R.Margin.reset()
            logits = model(dict(batch, feat=batch["feat"].to(dtype)), tables)
            loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
            loss.backward()
            runs.append((_collect(model, logits.detach(), loss.detach()), R.Margin.value))
        _REF["model"] = runs
    return _REF["model"]


@pytest.mark.parametrize("path", ["hip", "torch"])
def test_model_step_against_float64(path, monkeypatch):
    monkeypatch.setenv("AO_AMD_SPUNET", path)
    (f64, margin), (f32, _) = _device_reference()
    assert margin > SC.MARGIN, "the batch puts a ReLU pre-activation %.2e from its kink" % margin
    model, batch = _model(), _batch()
    logits, loss = _step(model, batch)
    assert tuple(logits.shape) == (3424, 13)
    got = _collect(model, logits, loss)
    assert len([k for k in got if k.startswith("g:")]) == len(list(model.parameters()))
    print("spunet-case model", path)
    _compare(M_MODEL, got, f64, f32, {"logits"})


def test_rows_come_back_in_input_order():
    """a permutation of the input rows permutes the output rows and nothing else (eval mode: the sums of a training-mode
    BatchNorm depend on the row order in the last place)"""
    model, batch = _model().eval(), _batch()
    n = batch["feat"].shape[0]
    perm = np.concatenate([np.random.default_rng(1).permutation(2130), 2130 + np.random.default_rng(2).permutation(n - 2130)])
    perm = torch.from_numpy(perm).cuda()
    with torch.no_grad():
        a = model(batch)
        b = model(dict(batch, discrete_coord=batch["discrete_coord"][perm], feat=batch["feat"][perm]))
    err = float((b - a[perm]).abs().max() / a.abs().max())
    print("spunet-equivariance largest difference over largest logit %.3e" % err)
    # the coarse levels are the same rows in the same order and every sum runs over kappa in the same order, so only a row
    # GEMM that rounds a row differently at another position can differ, in the last places; rows in a wrong order differ by
    # the size of the logits themselves
    assert err <= 1e-5


def test_one_table_build_per_forward(monkeypatch):
    from ao_amd.spunet import tables

    model, batch = _model(), _batch()
    calls = []
    real = torch.Tensor.tolist
    before = tables.BUILDS
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (calls.append(tuple(self.shape)), real(self))[1])
    _step(model, batch)
    monkeypatch.undo()
    assert tables.BUILDS - before == 1, "one table build serves the encoder and the decoder"
    assert calls == [(8,)], "one read-back: the five counts and the three status words"


def test_num_classes_0_returns_the_features():
    model, batch = _model(0).eval(), _batch()
    with torch.no_grad():
        feat = model(batch)
    assert tuple(feat.shape) == (3424, 96) and torch.isfinite(feat).all() and float(feat.min()) >= 0.0


def _segmentor_step(make):
    batch = _batch()
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        seg = make().cuda().train()
        out = seg(batch)
        out["loss"].backward()
        runs.append((out["loss"].detach(), {k: p.grad.clone() for k, p in seg.named_parameters() if p.grad is not None}))
        assert torch.isfinite(out["loss"])
        assert len(runs[-1][1]) == len(list(seg.parameters()))
        for key, g in runs[-1][1].items():
            assert torch.isfinite(g).all(), key
    assert torch.equal(runs[0][0], runs[1][0])
    for key in runs[0][1]:
        assert torch.equal(runs[0][1][key], runs[1][1][key]), key


def test_default_segmentor_trains_one_step(monkeypatch):
    from ao_amd.ptv2.segmentor import DefaultSegmentor

    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    _segmentor_step(lambda: DefaultSegmentor(backbone=_model(13)))


def test_cac_segmentor_trains_one_step(monkeypatch):
    from ao_amd.ptv2.cac import CACSegmentor

    monkeypatch.setenv("AO_AMD_SPUNET", "hip")
    _segmentor_step(lambda: CACSegmentor(13, 96, backbone=_model(0)))
