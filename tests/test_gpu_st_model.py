"""GPU: ao_amd.stratified.StratifiedTransformer against the float64 fixtures the reference's model produced on the CPU
(tests/golden/st_model_st2.npz, st_model_st3.npz; tests/golden/make_golden_st.py), in train and eval mode, on the three paths.

The pair sets of every block are compared exactly.  Logits, loss and the gradient of every parameter of at most 4096 elements
follow the rule of tests/test_gpu_st_ops.py with e_eager taken from the fixture: e_model <= M * max(e_eager, 2^-24), e_eager the
distance of the reference's own fp32 run from its float64 run.  Five biases stand in front of a normalisation and have true
gradient zero: they are bounded by M x the fp32 run's absolute noise.  M: twice the worst ratio measured on the MI355X over both
batches and the three paths, rounded up to a power of two."""
import os

import numpy as np
import pytest
import torch

from tests import st_cases as SC
from tests.test_gpu_st_ops import FLOOR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO_GRADS = {"g:up.1.linear1.0.bias", "g:up.1.linear1.1.bias", "g:up.1.linear2.0.bias", "g:up.1.linear2.1.bias", "g:classifier.0.bias"}
M_LOGITS, M_LOSS, M_GRAD, M_ZERO = 4, 4, 8, 4

_FIXTURES = {}


def fixture(name):
    if name not in _FIXTURES:
        z = np.load(os.path.join(GOLDEN, "st_model_%s.npz" % name))
        _FIXTURES[name] = {k: z[k] for k in z.files}
    return _FIXTURES[name]


def make_model():
    from ao_amd.stratified import StratifiedTransformer

    model = StratifiedTransformer(**SC.MODEL_CONFIG)
    state = SC.fill_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith(("K_points", "num_batches_tracked")) for k in missing.missing_keys)
    return model.cuda()


def batch_of(name):
    return {k: torch.from_numpy(v).cuda() for k, v in SC.model_batch(name).items()}


def _rel(a, ref):
    ref = torch.from_numpy(np.asarray(ref)).double()
    return float((a.detach().double().cpu() - ref).norm() / ref.norm())


def _peak(a, ref):
    ref = torch.from_numpy(np.asarray(ref)).double()
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _report(bad, tag, key, got, eager, m, floor=FLOOR):
    print("st-ratio model/%-12s %-48s kernel %.3e  eager %.3e  ratio %.3f" % (tag, key, got, eager, got / max(eager, floor)))
    if not got <= m * max(eager, floor):
        bad.append((key, got, eager))


@pytest.mark.parametrize("path", ["fused", "staged", "torch"])
@pytest.mark.parametrize("name", list(SC.MODEL_CLOUDS))
def test_training_step_against_the_float64_fixture(name, path, monkeypatch):
    from ao_amd.stratified import ops

    monkeypatch.setenv("AO_AMD_ST", path)
    z, batch, model = fixture(name), batch_of(name), make_model().train()
    seen = []
    inner = ops.window_attention
    monkeypatch.setattr(ops, "window_attention", lambda q, k, v, coords, pairs, *rest: (seen.append(pairs), inner(q, k, v, coords, pairs, *rest))[1])
    logits = model(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"]))
    loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
    loss.backward()
    # the pairs of every block, exactly
    assert len(seen) == sum(SC.MODEL_CONFIG["depths"])
    for i, pairs in enumerate(seen):
        ours = torch.stack([pairs.index_0, pairs.index_1.long()], 1).cpu().numpy()
        want = z["pairs/%d" % i].astype(np.int64)
        assert np.array_equal(ours[np.lexsort((ours[:, 1], ours[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))]), i
    bad, tag = [], "%s/%s" % (name, path)
    _report(bad, tag, "logits", _rel(logits, z["f64/logits"]), float(z["dist/logits"]), M_LOGITS)
    _report(bad, tag, "logits peak", _peak(logits, z["f64/logits"]), float(z["peak/logits"]), M_LOGITS)
    _report(bad, tag, "loss", _rel(loss, z["f64/loss"]), float(z["dist/loss"]), M_LOSS)
    want_keys = {k[4:] for k in z if k.startswith("f64/g:")}
    params = dict(model.named_parameters())
    have_keys = {"g:" + k for k, p in params.items() if p.grad is not None and p.numel() <= SC.SMALL_PARAMETER}
    assert have_keys == want_keys
    for key in sorted(want_keys):
        g = params[key[2:]].grad
        assert torch.isfinite(g).all(), key
        if key in ZERO_GRADS:
            _report(bad, tag, key, float(g.double().norm()), float(z["adist/" + key]), M_ZERO, 1e-30)
        else:
            _report(bad, tag, key, _rel(g, z["f64/" + key]), float(z["dist/" + key]), M_GRAD)
    assert not bad, bad


@pytest.mark.parametrize("path", ["fused", "staged", "torch"])
@pytest.mark.parametrize("name", list(SC.MODEL_CLOUDS))
def test_eval_logits_against_the_float64_fixture(name, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_ST", path)
    z, batch, model = fixture(name), batch_of(name), make_model().eval()
    with torch.no_grad():
        logits = model(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"]))
    bad, tag = [], "%s/%s/eval" % (name, path)
    _report(bad, tag, "eval_logits", _rel(logits, z["f64/eval_logits"]), float(z["dist/eval_logits"]), M_LOGITS)
    _report(bad, tag, "eval_logits peak", _peak(logits, z["f64/eval_logits"]), float(z["peak/eval_logits"]), M_LOGITS)
    assert not bad, bad


def test_a_supplied_neighbor_idx_is_used():
    from ao_amd import stratified

    batch, model = batch_of("st2"), make_model().eval()
    nbr = stratified.ball_query(SC.MODEL_CONFIG["kp_ball_radius"], SC.MODEL_CONFIG["kp_max_neighbor"], batch["coord"], batch["offset"])
    with torch.no_grad():
        a = model(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"]))
        b = model(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"], neighbor_idx=nbr))
    assert torch.equal(a, b)
