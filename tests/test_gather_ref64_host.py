"""CPU: what the comparisons of tests/test_gpu_gather_f64.py rest on.

1. The reference.  The float64 statements of tests/gather_ref64.py reproduce the committed fixtures that came from the
   reference's own python over the C oracle (grouping / interpolation / subtraction / aggregation / attention .npz) to the
   tolerances tests/test_gpu_ops.py holds the kernels to, agree with the oracle's autograd functions on random cases within
   the rounding-tier bound (the oracle is an fp32 sum in a fixed order: it has to obey it), and the pooling statements equal a
   plain per-cluster loop.
2. The bound.  The fp32 emulation of every summed contract (fp32 terms, added one after the other) stays within
   (T + 2) 2^-24 A in a random, an ascending-magnitude and a descending-magnitude order; on the exact tier every order returns
   float32(value) bit for bit, and the inputs satisfy the integer condition (asserted by the case builder).
3. Sensitivity.  Each deliberately wrong emulation -- last neighbour dropped, idx row shifted by one, ci / (c / w_c) for
   ci % w_c, tie to the last member, weight normalised by k, r % k for r / k in the gather backward -- violates the bound in at
   least one element of every rounding-tier case it changes and breaks bit equality on the exact tier."""
import numpy as np
import pytest
import torch

from oracle import pointops_ref as P
from tests import gather_cases as C
from tests import gather_ref64 as R

F32, F64 = np.float32, np.float64
LAUNCHERS = list(C.CASES)


def _small(launcher):
    return [(case, tier) for case, tier in C.pairs(launcher) if "big" not in case.flags]


def _close(got, want, tol):
    np.testing.assert_allclose(np.asarray(got, F64), want, rtol=tol, atol=tol)


# ------------------------------------------------------------------------------------------------------------- 1. the reference
def test_statements_reproduce_the_reference_fixtures(golden):
    g = golden("grouping.npz")
    out = R.grouping_forward(dict(input=g["feat"], idx=g["idx"]))["output"]
    assert np.array_equal(out.astype(F32), g["out2"])
    _close(R.grouping_backward(dict(grad_output=g["grad_out2"], idx=g["idx"], n=160))["grad_input"].value, g["grad_feat2"], 1e-5)
    out = R.grouping_forward(dict(input=g["feat"], idx=g["idx_m1"]))["output"]     # the feature half of grouping(with_xyz=True)
    assert (g["idx_m1"] < 0).any()
    _close(out, g["out_xyz"][..., 3:], 1e-6)
    _close(R.grouping_backward(dict(grad_output=g["grad_out"][..., 3:], idx=g["idx_m1"], n=160))["grad_input"].value,
           g["grad_feat"], 1e-5)

    g = golden("interpolation.npz")
    idx, d2 = P.knn_query_raw(3, torch.from_numpy(g["xyz"]), torch.from_numpy(g["offset"]), torch.from_numpy(g["new_xyz"]),
                              torch.from_numpy(g["new_offset"]))
    w = R.interpolation_weights(dict(dist2=d2.numpy(), idx=idx.numpy(), n=50))
    t = dict(input=g["feat"], idx=w["idx"], weight=w["weight"].astype(F32), grad_output=g["grad_out"], m=50)
    _close(R.interpolation_forward(t)["output"].value, g["out"], 1e-5)
    _close(R.interpolation_backward(t)["grad_input"].value, g["grad_feat"], 1e-4)

    g = golden("subtraction.npz")
    t = dict(input1=g["in1"], input2=g["in2"], idx=g["idx"], grad_output=g["grad_out"])
    assert np.array_equal(R.subtraction_forward(t)["output"].astype(F32), g["out"])
    back = R.subtraction_backward(t)
    _close(back["grad_input1"].value, g["grad_in1"], 1e-5)
    _close(back["grad_input2"].value, g["grad_in2"], 1e-5)

    g = golden("aggregation.npz")
    t = {k: g[k] for k in ("input", "position", "weight", "idx")}
    t["grad_output"] = g["grad_out"]
    _close(R.aggregation_forward(t)["output"].value, g["out"], 1e-5)
    back = R.aggregation_backward(t)
    _close(back["grad_input"].value, g["grad_input"], 1e-4)
    _close(back["grad_position"], g["grad_position"], 1e-6)
    _close(back["grad_weight"].value, g["grad_weight"], 1e-4)

    g = golden("attention.npz")
    t = {k: g[k] for k in ("query", "key", "weight", "index_target", "index_refer")}
    t["grad_output"] = g["grad_relation"]
    _close(R.attention_relation_step_forward(t)["output"].value, g["relation"], 1e-5)
    back = R.attention_relation_step_backward(t)
    _close(back["grad_query"].value, g["grad_query"], 1e-4)
    _close(back["grad_key"].value, g["grad_key"], 1e-4)
    t = dict(weight=g["attn"], value=g["value"], index_target=g["index_target"], index_refer=g["index_refer"],
             grad_output=g["grad_fused"])
    _close(R.attention_fusion_step_forward(t)["output"].value, g["fused"], 1e-5)
    back = R.attention_fusion_step_backward(t)
    _close(back["grad_weight"].value, g["grad_attn"], 1e-4)
    _close(back["grad_value"].value, g["grad_value"], 1e-4)


def _within(got, ref, what):
    ok, ratio, msg = R.compare(np.ascontiguousarray(got.numpy() if hasattr(got, "numpy") else got), ref, "rounding")
    assert ok, (what, ratio, msg)


def _tt(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.requires_grad_(True) if grad else x


@pytest.mark.parametrize("pick", [5, 6])
def test_statements_agree_with_the_oracle_autograd_functions(pick):
    """the oracle (oracle/pointops_oracle.c) is fp32 in a fixed order without contraction: it obeys the rounding-tier bound"""
    tier = "rounding"
    case = C.CASES["grouping_backward_hip_launcher"][pick]
    t, ref, _ = C.inputs(case, tier)
    x = _tt(C.inputs(C.CASES["grouping_forward_hip_launcher"][pick], tier)[0]["input"], True)
    idx = np.maximum(t["idx"], 0)   # the reference's grouping2 has no -1 handling
    out = P.grouping2(x, _tt(idx))
    assert R.bits_equal(out.detach().numpy(), R.grouping_forward(dict(input=x.detach().numpy(), idx=idx))["output"].astype(F32))
    (gx,) = torch.autograd.grad(out, x, _tt(t["grad_output"]))
    _within(gx, R.grouping_backward(dict(t, idx=idx))["grad_input"], "grouping")

    t, ref, _ = C.inputs(C.CASES["subtraction_backward_hip_launcher"][pick], tier)
    f = C.inputs(C.CASES["subtraction_forward_hip_launcher"][pick], tier)[0]
    a, b = _tt(f["input1"], True), _tt(f["input2"], True)
    out = P.subtraction(a, b, _tt(f["idx"]))
    assert R.bits_equal(out.detach().numpy(), R.subtraction_forward(f)["output"].astype(F32))
    ga, gb = torch.autograd.grad(out, (a, b), _tt(t["grad_output"]))
    back = R.subtraction_backward(dict(t, idx=f["idx"]))
    _within(ga, back["grad_input1"], "subtraction 1")
    _within(gb, back["grad_input2"], "subtraction 2")

    t, ref, _ = C.inputs(C.CASES["aggregation_backward_hip_launcher"][pick], tier)
    x, p, w = (_tt(t[k], True) for k in ("input", "position", "weight"))
    out = P.aggregation(x, p, w, _tt(t["idx"]))
    _within(out.detach(), R.aggregation_forward(t)["output"], "aggregation")
    grads = torch.autograd.grad(out, (x, p, w), _tt(t["grad_output"]))
    for got, key in zip(grads, ("grad_input", "grad_position", "grad_weight")):
        _within(got, ref[key], "aggregation " + key)

    t, ref, _ = C.inputs(C.CASES["attention_relation_step_backward_hip_launcher"][pick - 2], tier)
    q, k = _tt(t["query"], True), _tt(t["key"], True)
    out = P.attention_relation_step(q, k, _tt(t["weight"]), _tt(t["index_target"]), _tt(t["index_refer"]))
    _within(out.detach(), R.attention_relation_step_forward(t)["output"], "relation")
    gq, gk = torch.autograd.grad(out, (q, k), _tt(t["grad_output"]))
    _within(gq, ref["grad_query"], "relation grad_query")
    _within(gk, ref["grad_key"], "relation grad_key")

    t, ref, _ = C.inputs(C.CASES["attention_fusion_step_backward_hip_launcher"][pick - 2], tier)
    w, v = _tt(t["weight"], True), _tt(t["value"], True)
    out = P.attention_fusion_step(w, v, _tt(t["index_target"]), _tt(t["index_refer"]))
    _within(out.detach(), R.attention_fusion_step_forward(t)["output"], "fusion")
    gw, gv = torch.autograd.grad(out, (w, v), _tt(t["grad_output"]))
    _within(gw, ref["grad_weight"], "fusion grad_weight")
    _within(gv, ref["grad_value"], "fusion grad_value")


@pytest.mark.parametrize("k,seed", [(3, 0), (5, 1)])
def test_interpolation_statements_agree_with_the_oracle(k, seed):
    rng = np.random.default_rng(seed)
    xyz, new_xyz = rng.random((40, 3)).astype(F32), rng.random((130, 3)).astype(F32)
    off, new_off = np.array([15, 40], np.int32), np.array([50, 130], np.int32)   # (interpolation2 does not wrap a -1: none here)
    feat = _tt(rng.standard_normal((40, 7)).astype(F32), True)
    go = rng.standard_normal((130, 7)).astype(F32)
    out = P.interpolation2(_tt(xyz), _tt(new_xyz), feat, _tt(off), _tt(new_off), k)
    (gf,) = torch.autograd.grad(out, feat, _tt(go))
    idx, d2 = P.knn_query_raw(k, _tt(xyz), _tt(off), _tt(new_xyz), _tt(new_off))
    assert (idx >= 0).all()
    w = R.interpolation_weights(dict(dist2=d2.numpy(), idx=idx.numpy(), n=40))
    _, ow = P.interpolation_weights(_tt(xyz), _tt(new_xyz), _tt(off), _tt(new_off), k)   # through sqrt'ed distances, torch.sum
    assert np.abs(ow.numpy() - w["weight"]).max() <= (k + 6) * R.U
    # the oracle's forward / backward on ITS weights against the statements on the same weights
    t = dict(input=feat.detach().numpy(), idx=w["idx"], weight=ow.numpy(), grad_output=go, m=40)
    _within(out.detach(), R.interpolation_forward(t)["output"], "interpolation")
    _within(gf, R.interpolation_backward(t)["grad_input"], "interpolation backward")


@pytest.mark.parametrize("pick", [5, 10])
def test_pooling_statements_equal_a_per_cluster_loop(pick):
    for tier in C.TIERS:
        t, _, _ = C.inputs(C.CASES["pool_max_forward_hip_launcher"][pick], tier)
        ref = R.pool_max_forward(t)
        order, ptr, feat = t["order"], t["idx_ptr"], t["feat"]
        for j in range(ptr.size - 1):
            rows = order[ptr[j]:ptr[j + 1]]
            for ch in range(feat.shape[1]):
                col = feat[rows, ch]
                best = int(np.flatnonzero(col == col.max())[0])                  # the first member among the maxima
                assert ref["arg"][j, ch] == rows[best]
                assert R.bits_equal(ref["out"][j, ch].astype(F32).reshape(1), col[best].reshape(1))
        b, _, _ = C.inputs(C.CASES["pool_max_backward_hip_launcher"][pick if pick < 10 else 5], tier)
        gf = np.zeros((b["n_in"], b["grad_out"].shape[1]))
        for j in range(b["arg"].shape[0]):
            for ch in range(b["arg"].shape[1]):
                gf[b["arg"][j, ch], ch] = b["grad_out"][j, ch]
        assert np.array_equal(R.pool_max_backward(b)["grad_feat"], gf)
        s, sref, _ = C.inputs(C.CASES["segment_sum_hip_launcher"][pick if pick < 10 else 5], tier)
        want = np.stack([s["grad_fine"][s["order"][s["idx_ptr"][j]:s["idx_ptr"][j + 1]]].astype(F64).sum(0)
                         for j in range(s["idx_ptr"].size - 1)])
        _close(sref["grad_coarse"].value, want, 1e-14)
        assert np.array_equal(sref["grad_coarse"].T[:, 0], np.diff(s["idx_ptr"]))
    for case in C.CASES["segment_minmax_hip_launcher"]:
        t, ref, _ = C.inputs(case, "rounding")
        for s, (a, b) in enumerate(zip(np.r_[0, t["offset"][:-1]], t["offset"])):
            assert np.array_equal(ref["lo"][s], t["xyz"][a:b].min(0)) and np.array_equal(ref["hi"][s], t["xyz"][a:b].max(0))


def test_case_lists_hold_what_they_promise():
    assert len(C.CASES) == 18 == len(R.CONTRACTS) == len(R.KEYS) == len(R.MUTANTS)
    for launcher, cases in C.CASES.items():
        assert len({c.name for c in cases}) == len(cases)
        if launcher == "segment_minmax_hip_launcher":   # a fixed grid of 64 chunks per cloud: its second trip is a cloud above 16 384
            continue
        big = [c for c in cases if "big" in c.flags]
        assert len(big) == 1, launcher
        cap = C.second_trip_threads(launcher)
        assert cap < C.threads(big[0]) <= cap + 1024, (launcher, C.threads(big[0]), cap)   # just above: a second trip
        assert all(C.threads(c) <= cap for c in cases if "big" not in c.flags)
    for name in ("grouping_backward", "aggregation_backward", "attention_relation_step_backward", "attention_fusion_step_forward",
                 "attention_relation_step_forward", "attention_fusion_step_backward"):
        assert any("contention" in c.flags for c in C.CASES[name + "_hip_launcher"]), name
    # inverse lists of 0, 1, 2, 8, 9, 10, 17, 18 entries; rows nobody points at with m < n
    case = next(c for c in C.CASES["interpolation_backward_gather_hip_launcher"] if c.name == "r257-s9-c48")
    t, ref, _ = C.inputs(case, "rounding")
    assert t["m"] < 257 and tuple(np.bincount(t["idx"].ravel(), minlength=t["m"])[:8]) == C.PLANTED
    assert tuple(ref["grad_input"].T[:8, 0]) == C.PLANTED
    atomic = next(c for c in C.CASES["interpolation_backward_hip_launcher"] if c.name == case.name)   # the same idx and weights
    ta, refa, _ = C.inputs(atomic, "rounding")
    assert all(np.array_equal(t[k], ta[k]) for k in ("idx", "weight", "grad_output")) and t["m"] == ta["m"]
    t, _, _ = C.inputs(next(c for c in C.CASES["pool_max_forward_hip_launcher"] if c.name == "j257-c48-ties"), "rounding")
    assert set(C.CLUSTER_LENGTHS) <= set(np.diff(t["idx_ptr"])) and (np.diff(t["order"]) < 0).any()
    sizes = [c.p["sizes"] for c in C.CASES["segment_minmax_hip_launcher"]]
    assert any(max(s) > 16384 for s in sizes) and any(1 in s for s in sizes) and {len(s) for s in sizes} == {1, 3}


# ---------------------------------------------------------------------------------------------------------------- 2. the bound
@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_fp32_emulation_stays_within_the_bound_in_three_orders(launcher):
    rng = np.random.default_rng(1)
    summed = 0
    for case, tier in _small(launcher):
        t, ref, bits = C.inputs(case, tier)
        assert set(ref) == set(R.KEYS[launcher])
        emu = R.CONTRACTS[launcher](t, F32)
        for order in ("random", "ascending", "descending") if tier == "rounding" else ("random", "descending"):
            got = R.realise(emu, order, rng)
            for key in R.KEYS[launcher]:
                if launcher == "interpolation_weights_hip_launcher" and key == "weight" and tier == "rounding":
                    ok, ratio, msg = R.compare_weights(got[key], ref[key], case.p["ns"])
                else:
                    ok, ratio, msg = R.compare(got[key].astype(F32) if got[key].dtype == F64 else got[key], ref[key], tier)
                assert ok, (launcher, case.name, tier, order, key, ratio, msg)
                summed += isinstance(ref[key], R.Sum)
    assert summed or launcher in ("grouping_forward_hip_launcher", "subtraction_forward_hip_launcher", "segment_minmax_hip_launcher",
                                  "pool_max_forward_hip_launcher", "pool_max_backward_hip_launcher",
                                  "interpolation_weights_hip_launcher")


def test_bound_on_long_random_sums():
    """the bound itself, apart from any contract: sums of T = 2 ... 400 products in the three orders"""
    rng = np.random.default_rng(2)
    worst = 0.0
    for terms in (2, 3, 17, 100, 400):
        a, b = rng.standard_normal((500, terms)).astype(F32), rng.standard_normal((500, terms)).astype(F32)
        dest = np.repeat(np.arange(500), terms)
        s64 = R.Sum((500,), dest, a.astype(F64) * b.astype(F64), 2, 1)
        s32 = R.Sum((500,), dest, a * b, 2, 1)
        for order in ("random", "ascending", "descending"):
            err = np.abs(R.emulate(s32, order, rng).astype(F64) - s64.value)
            assert (err <= s64.bound()).all()
            worst = max(worst, float((err / s64.bound()).max()))
    assert 0.0 < worst < 1.0


def test_second_trip_cases_satisfy_the_integer_condition():
    for launcher, cases in C.CASES.items():
        case = next((c for c in cases if "big" in c.flags), None)
        if case is None:
            assert launcher == "segment_minmax_hip_launcher"
            continue
        t, ref, bits = C.inputs(case, "exact")     # (the builder asserts A 2^f integer < 2^24 for the bits it returns)
        assert 0 <= bits <= 3 and C.check_exact(ref, bits), (launcher, case.name)


# ------------------------------------------------------------------------------------------------------------- 3. sensitivity
def applies(case, tier, t, mut):
    """does the mutation change what the contract computes on this case"""
    p, name = case.p, case.launcher
    if mut == "tie_last":
        return "ties" in case.flags
    if mut == "wc_div":
        w_c, c = t["weight"].shape[2], p["c"]
        return p["rows"] > 0 and 1 < w_c < c
    if mut == "norm_k":
        return p["rows"] > 0 and p["ns"] >= 2
    if mut == "r_mod_k":
        return p["rows"] >= 2 and p["ns"] >= 2
    if mut == "shift":
        keys = [k for k in ("idx", "index_target", "index_refer", "arg") if k in t]
        return any(not np.array_equal(np.roll(t[k], 1, axis=0), t[k]) for k in keys)
    if name in ("pool_max_forward_hip_launcher", "segment_sum_hip_launcher"):
        return bool((np.diff(t["idx_ptr"]) >= 2).any())
    if name == "segment_minmax_hip_launcher":
        return max(p["sizes"]) >= 2
    if name.startswith("attention_"):
        return p["m"] > 0 and (p["c"] if ("relation_step_forward" in name or "fusion_step_backward" in name) else p["m"]) >= 1
    return p["rows"] > 0


@pytest.mark.parametrize("launcher", LAUNCHERS)
def test_wrong_emulations_are_caught(launcher):
    rng = np.random.default_rng(3)
    fn = R.CONTRACTS[launcher]
    ran = {m: 0 for m in R.MUTANTS[launcher]}
    for case, tier in _small(launcher):
        t, ref, bits = C.inputs(case, tier)
        for mut in R.MUTANTS[launcher]:
            if not applies(case, tier, t, mut):
                continue
            got = R.realise(fn(t, F32 if tier == "rounding" else F64, mut), "random", rng)
            caught = False
            for key in R.KEYS[launcher]:
                g = got[key].astype(F32) if got[key].dtype == F64 else got[key]
                if launcher == "interpolation_weights_hip_launcher" and key == "weight" and tier == "rounding":
                    ok = R.compare_weights(g, ref[key], case.p["ns"])[0]
                elif tier == "rounding" and isinstance(ref[key], R.Sum):
                    ok = bool((np.abs(g.astype(F64) - ref[key].value) <= ref[key].bound()).all())   # the bound alone
                else:
                    ok = R.compare(g, ref[key], tier)[0]
                caught |= not ok
            assert caught, (launcher, case.name, tier, mut, "not noticed")
            ran[mut] += 1
    assert all(ran.values()), ran
