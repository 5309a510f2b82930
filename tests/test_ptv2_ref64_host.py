"""CPU: the float64 reference of the PT-v2m2 Block and model (tests/ptv2_ref64.py), the recorded seeds
(tests/ptv2_f64_cases.py) and the comparison that tests/test_gpu_ptv2_f64.py applies to the native runtimes.

  * the model restatement on given tables, in float32 on the oracle's tables, equals oracle.ptv2_ref.forward bit for bit;
  * every recorded seed meets the margin condition (a case that does not is an error);
  * the compared key set is every parameter and every buffer of the module, and the keys treated as exactly zero are exactly
    the gradients that vanish in float64;
  * mutation checks: the eager float32 result with one subtle defect put in fails the comparison at the largest M any class
    of output may ever be given (ptv2_ref64.M_CAP)."""
import pytest
import torch

from oracle import pointops_ref as P
from oracle import ptv2_ref as M
from tests import ptv2_f64_cases as C
from tests import ptv2_ref64 as R

M_MAX = {k: R.M_CAP for k in ("out", "logits", "loss", "g_x", "grad", "buffer", "zero")}
_RUNS = {}


def _block_run(name, mode):
    key = ("block", name, mode)
    if key not in _RUNS:
        case = C.BLOCK_CASES[name]
        coord, offset = (torch.from_numpy(a) for a in C.block_cloud(name))
        idx = P.knn_query(case.k, coord, offset)[0]
        _RUNS[key] = C.block_reference(name, mode, C.BLOCK_SEEDS[name, mode], coord, idx) + (coord, idx)
    return _RUNS[key]


def _model_run(name):
    key = ("model", name)
    if key not in _RUNS:
        case, cfg = C.MODEL_CASES[name], C.model_cfg(name)
        coord, offset = (torch.from_numpy(a) for a in C.model_cloud(case.clouds))
        levels = R.oracle_tables(cfg, coord, offset)
        _RUNS[key] = C.model_reference(cfg, case.training, C.MODEL_SEEDS[name], coord, levels) + (coord, levels)
    return _RUNS[key]


BLOCK_IDS = [(n, m) for n, c in C.BLOCK_CASES.items() for m in c.modes]


# ----------------------------------------------------------------------------------------------------- the restatement ----
@pytest.mark.parametrize("backend", ["interp", "map"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_restatement_equals_the_oracle_forward_bit_for_bit(backend, training):
    cfg = C.skeleton(0, unpool_backend=backend, patch_embed_depth=1, enc_depths=(1, 1), dec_depths=(1, 1))
    coord, offset = (torch.from_numpy(a) for a in C.model_cloud())
    inp = C.model_inputs(cfg, 3, coord.numpy())
    want = M.forward(inp["state"], cfg, coord, inp["feat"], offset, training=training)
    levels = R.oracle_tables(cfg, coord, offset)
    with torch.no_grad():
        got = R.forward_tables(M.Ctx(inp["state"], training), cfg, inp["feat"], levels)
    assert torch.equal(got, want)
    res, rec = R.run_model(inp["state"], cfg, inp["feat"], levels, inp["segment"], training, torch.float32, grads=False)
    assert torch.equal(res["logits"], want)  # the recorded run is the same run
    assert len(rec.pools) == 2 and len(rec.pre) == 1 + 5 * 7 + 2 + 4 + 1


def test_recorder_finds_the_gap_and_the_runner_up():
    d = torch.tensor([[1.0, 0.0], [3.0, 0.0], [2.5, 0.0], [7.0, 4.0]])
    rec = R.Recorder()
    rec.pool(d, torch.tensor([2, 0, 1, 3]), torch.tensor([0, 3, 4]))
    p = rec.pools[0]
    assert p["gap"][0].tolist() == [0.5, float("inf")]          # 3.0 - 2.5; 0 / 0 is exempt
    assert p["gap"][1].tolist() == [float("inf"), float("inf")]  # one member
    assert int(p["first"][0, 0]) == 1 and int(p["second"][0, 0]) == 2


# ------------------------------------------------------------------------------------------------------------ the seeds ----
def test_every_case_has_a_recorded_seed():
    assert set(C.BLOCK_SEEDS) == set(BLOCK_IDS) and set(C.MODEL_SEEDS) == set(C.MODEL_CASES)


@pytest.mark.parametrize("name,mode", BLOCK_IDS)
def test_block_seed_meets_the_margin(name, mode):
    small, eps = _block_run(name, mode)[2]
    assert small >= R.RATIO * eps, "ratio %.2f" % (small / eps)


@pytest.mark.parametrize("name", list(C.MODEL_CASES))
def test_model_seed_meets_the_margin(name):
    small, eps = _model_run(name)[2]
    assert small >= R.RATIO * eps, "ratio %.2f" % (small / eps)


# ------------------------------------------------------------------------------------------------------------- the keys ----
def _vanishing(f64):
    """the gradient keys whose float64 norm is below 1e-9 of their layer's weight gradient"""
    out = set()
    for k, v in f64.items():
        if k.startswith("g:") and k.endswith(".bias") and ".norm." not in k:
            if float(v.norm()) <= 1e-9 * float(f64[k[: -len("bias")] + "weight"].norm()):
                out.add(k)
    return out


@pytest.mark.parametrize("name,mode", BLOCK_IDS)
def test_block_keys_are_complete_and_the_zero_keys_are_the_vanishing_gradients(name, mode):
    from ao_amd.ptv2.model import Block

    case = C.BLOCK_CASES[name]
    f64, f32, _, _, _, idx = _block_run(name, mode)
    blk = Block(case.c, case.g, qkv_bias=case.qkv_bias)
    want = {"out", "g_x"} | {"g:" + k for k, _ in blk.named_parameters()} | {"b:" + k for k, _ in blk.named_buffers()}
    assert set(f64) == set(f32) == want
    names = [k for k, _ in blk.named_parameters()]
    assert _vanishing(f64) == set(R.zero_keys(names, mode == "train", masked=bool((idx < 0).any())))
    assert bool((idx < 0).any()) == (name == "short_clouds")


@pytest.mark.parametrize("name", list(C.MODEL_CASES))
def test_model_keys_are_complete_and_the_zero_keys_are_the_vanishing_gradients(name):
    from ao_amd.ptv2.model import PointTransformerV2

    case, cfg = C.MODEL_CASES[name], C.model_cfg(name)
    f64, f32, _, _, _, levels = _model_run(name)
    model = PointTransformerV2(**cfg)
    want = {"logits", "loss"} | {"g:" + k for k, _ in model.named_parameters()} | {"b:" + k for k, _ in model.named_buffers()}
    assert set(f64) == set(f32) == want
    assert sum(len(s.blocks) for s in [model.patch_embed.blocks] + [e.blocks for e in model.enc_stages]
               + [d.blocks for d in model.dec_stages]) == 1
    level = [0, 1, 2, 0, 1][case.seq]
    masked = bool((levels[level]["knn"][16] < 0).any())
    assert _vanishing(f64) == set(R.zero_keys([k for k, _ in model.named_parameters()], case.training, masked=masked))


# -------------------------------------------------------------------------------------------------------- the mutations ----
def _misses(got, f64, f32, zeros):
    return {name for name, _, _ in R.compare(M_MAX, got, f64, f32, zeros, "host")}


def _block_zeros(name, mode, f64, idx):
    return R.zero_keys([k[2:] for k in f64 if k.startswith("g:")], mode == "train", masked=bool((idx < 0).any()))


def test_the_eager_run_itself_passes_at_m_1():
    f64, f32, _, _, _, idx = _block_run("c48", "train")
    ones = dict.fromkeys(M_MAX, 1)
    assert not R.compare(ones, f32, f64, f32, _block_zeros("c48", "train", f64, idx), "host")
    f64, f32 = _model_run("seq2")[:2]
    assert not R.compare(ones, f32, f64, f32, R.zero_keys([k[2:] for k in f64 if k.startswith("g:")], True, True), "host")


def test_mutation_batchnorm_weight_gradient_scaled_by_2_to_the_minus_12():
    f64, f32, _, _, _, idx = _block_run("c48", "train")
    got = dict(f32)
    got["g:norm2.norm.weight"] = f32["g:norm2.norm.weight"] * (1.0 + 2.0 ** -12)
    assert _misses(got, f64, f32, _block_zeros("c48", "train", f64, idx)) == {"g:norm2.norm.weight"}


def test_mutation_running_var_from_the_biased_variance():
    f64, f32, _, inp, _, idx = _block_run("c48", "train")
    n, key = inp["x"].shape[0], "norm1.norm.running_var"
    old = inp["state"][key]
    unbiased = (f32["b:" + key] - 0.9 * old) / 0.1
    got = dict(f32)
    got["b:" + key] = 0.9 * old + 0.1 * unbiased * (n - 1) / n
    assert _misses(got, f64, f32, _block_zeros("c48", "train", f64, idx)) == {"b:" + key}


def _block_without_the_droppath_factor_in_the_backward(cx, pre, feat, coord, ref_idx, groups):
    """oracle.ptv2_ref._block (:164-177) with the same values, whose branch gradient misses the DropPath factor"""
    F = M.F
    identity = feat
    feat = F.relu(M._pbn(cx, F.linear(feat, cx.s[pre + ".fc1.weight"]), pre + ".norm1"))
    feat = M._gva(cx, pre + ".attn", feat, coord, ref_idx, groups)
    feat = F.relu(M._pbn(cx, feat, pre + ".norm2"))
    feat = M._pbn(cx, F.linear(feat, cx.s[pre + ".fc3.weight"]), pre + ".norm3")
    feat = (feat * cx.drop_masks[pre]).detach() + (feat - feat.detach())
    return F.relu(identity + feat)


def test_mutation_droppath_factor_left_out_of_the_backward():
    f64, f32, _, inp, coord, idx = _block_run("rowscale", "train")
    with R.eager_host():
        got, _ = R.run_block(inp["state"], inp["x"], coord, idx, 6, inp["go"], True, inp["keep"], torch.float32,
                             block=_block_without_the_droppath_factor_in_the_backward)
    assert torch.equal(got["out"], f32["out"])
    missed = _misses(got, f64, f32, _block_zeros("rowscale", "train", f64, idx))
    assert "g_x" in missed and "out" not in missed and not any(k.startswith("b:") for k in missed)
    # the reference itself: a dropped row returns the identity, and a gradient that arrives at dropped rows alone reaches
    # no parameter (the branch gradient is 0)
    dropped = inp["keep"] == 0
    assert 0.3 < float(dropped.float().mean()) < 0.7
    assert torch.equal(f64["out"][dropped], inp["x"][dropped].double())


@pytest.mark.parametrize("mutation", ["drop_skip", "pool_second"])
def test_mutation_in_the_model_wiring(mutation):
    """one of the two contributions to the gradient of the level-0 skip tensor dropped; the gradient of one pooled value sent
    to the runner-up row"""
    f64, f32, _, inp, coord, levels = _model_run("seq2")
    cfg = C.model_cfg("seq2")
    with R.eager_host():
        got, _ = R.run_model(inp["state"], cfg, inp["feat"], levels, inp["segment"], True, torch.float32, mutate=(mutation,))
    assert torch.equal(got["logits"], f32["logits"]) and torch.equal(got["loss"], f32["loss"])
    masked = bool((levels[2]["knn"][16] < 0).any())
    missed = _misses(got, f64, f32, R.zero_keys([k[2:] for k in f64 if k.startswith("g:")], True, masked))
    assert "g:patch_embed.proj.0.weight" in missed
    assert not any(k.startswith(("b:", "logits", "loss", "g:seg_head", "g:dec_stages")) for k in missed)
