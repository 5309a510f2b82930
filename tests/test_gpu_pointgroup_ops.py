"""GPU: the operators of ao_amd/pointgroup/ops.py (ao_amd/csrc/pointgroup.hip) against tests/pointgroup_ref.py, on both paths
(HIP and AO_AMD_PG=torch) where both exist.

Ball query and clustering are integer-exact: the cases keep every pair at least pointgroup_cases.MARGIN * r^2 away from r^2
(or exactly on it, in exact arithmetic), because nobody has compared the rounding sequence of ref_d2() with what the
reference's compiler emits for its kernel.  Scores are held to (m + 8) * 2^-24 relative of float64 for a cluster of m members:
the worst case of any fp32 summation order of m non-negative terms, plus a few ulp for the softmax.  The offset losses and
their gradient are held to max(2 * the eager fp32 statements' error on the same GPU, 4 ulp of the value) against float64: two
legitimate summation orders differ."""
import numpy as np
import pytest
import torch

from tests import pointgroup_cases as C
from tests import pointgroup_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def _ball_ref(name):
    if name not in _REF:
        _REF[name] = R.ball_query(*C.ball_cases()[name])
    return _REF[name]


def _run_ball(name):
    from ao_amd import pointgroup

    coords, offsets, radius = C.ball_cases()[name]
    idx, start_len, capped = pointgroup.ball_query(torch.from_numpy(coords).cuda(), torch.from_numpy(offsets).cuda(), radius)
    assert idx.dtype == torch.int32 and start_len.dtype == torch.int32 and start_len.shape == (coords.shape[0], 2)
    return idx.cpu().numpy(), start_len.cpu().numpy(), capped


BALL = ["lattice_strict", "two_clouds", "empty_segment", "single", "cell_edges", "outlier", "random_margin", "cap", "cap_exact",
        "cap_1010"]


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", BALL)
def test_ball_query(name, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_PG", path)
    lists, ref_idx, ref_start_len, ref_capped = _ball_ref(name)
    idx, start_len, capped = _run_ball(name)
    n = len(lists)
    # start is the exclusive prefix sum of len in point order; nActive their sum
    assert np.array_equal(start_len[:, 1], ref_start_len[:, 1])
    assert np.array_equal(start_len[:, 0], np.cumsum(start_len[:, 1]) - start_len[:, 1])
    assert idx.shape[0] == int(start_len[:, 1].sum()) == ref_idx.shape[0]
    for p in range(n):
        assert np.array_equal(idx[start_len[p, 0]:start_len[p, 0] + start_len[p, 1]], lists[p]), (name, p)
    assert capped == ref_capped == (name in ("cap", "cap_1010"))
    if name.startswith("cap"):
        blob = {"cap": 1100, "cap_exact": 1000, "cap_1010": 1010}[name]
        is_blob = C.cap_case(blob)[3]
        lowest = np.nonzero(is_blob)[0][:1000].astype(np.int32)
        for p in np.nonzero(is_blob)[0][[0, 1, 500, blob - 1]]:
            assert np.array_equal(idx[start_len[p, 0]:start_len[p, 0] + start_len[p, 1]], lowest), "the 1 000 lowest blob indices"
        for p in np.nonzero(~is_blob)[0]:
            assert idx[start_len[p, 0]:start_len[p, 0] + start_len[p, 1]].tolist() == [p]
    if name == "two_clouds":
        assert (idx[:start_len[150, 0]] < 150).all() and (idx[start_len[150, 0]:] >= 150).all()
        assert np.array_equal(idx[start_len[150, 0]:] - 150, idx[:start_len[150, 0]])


def test_ballquery_batch_p_signature():
    """the reference's call: (coords, batch_idxs, batch_offsets, radius, meanActive) -> (idx, start_len); meanActive is unused"""
    from ao_amd import pointgroup

    coords, offsets, radius = C.ball_cases()["empty_segment"]
    batch = np.searchsorted(offsets[1:], np.arange(coords.shape[0]), side="right").astype(np.int32)
    args = (torch.from_numpy(coords).cuda(), torch.from_numpy(batch).cuda(), torch.from_numpy(offsets).cuda(), radius)
    idx, start_len = pointgroup.ballquery_batch_p(*args, 300)
    idx1, start_len1 = pointgroup.ballquery_batch_p(*args, 1)
    assert torch.equal(idx, idx1) and torch.equal(start_len, start_len1) and idx.is_cuda
    assert np.array_equal(idx.cpu().numpy(), _ball_ref("empty_segment")[1])


# ----------------------------------------------------------------------------------------------------------- clustering ----
@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", ["chain", "labels_touching", "threshold", "interleaved", "capped_directed", "all_ignored"])
def test_cluster(name, path, monkeypatch):
    from ao_amd import pointgroup

    monkeypatch.setenv("AO_AMD_PG", path)
    coords, offsets, radius, label, min_points = C.cluster_cases()[name]
    _, _, ref_capped, rows, coffsets, want = C.cluster_expected(name)
    idx, start_len, capped = pointgroup.ball_query(torch.from_numpy(coords).cuda(), torch.from_numpy(offsets).cuda(), radius)
    assert capped == ref_capped
    got, sizes, firsts = pointgroup.cluster(torch.from_numpy(label).cuda(), idx, start_len, min_points, capped)
    assert got.dtype == torch.int32 and got.is_cuda
    # the numbering of the reference's search: ascending smallest member; the same set per cluster
    assert np.array_equal(got.cpu().numpy(), want), name
    assert sizes.cpu().tolist() == np.diff(coffsets).tolist()
    assert firsts.cpu().tolist() == [int(rows[o, 1]) for o in coffsets[:-1]], "the first point of a cluster is the reference's"
    if name == "capped_directed":
        # a plain connected-components answer (one cluster of 1 100) fails here
        assert sizes.cpu().tolist() == [1000] and int((want >= 0).sum()) == 1000
        # the drop-in decides from start_len alone
        again, _, _ = pointgroup.cluster(torch.from_numpy(label).cuda(), idx, start_len, min_points)
        assert torch.equal(again, got)
    if name == "chain":
        assert firsts.cpu().tolist() == [0] and float(coords[0, 0]) == 100.0


# ------------------------------------------------------------------------------------------------------------ proposals ----
@pytest.mark.parametrize("form", ["hip-prob", "hip-logit", "torch"])
def test_proposals(form, monkeypatch):
    from ao_amd import pointgroup

    monkeypatch.setenv("AO_AMD_PG", "torch" if form == "torch" else "hip")
    point_cluster, sizes, firsts, rows, offsets, segment_pred, logits = C.proposal_case()
    n = point_cluster.shape[0]
    want_scores, want_masks, want_classes, members = R.proposals(rows, offsets, segment_pred, R.softmax64(logits), 100, n)
    assert sorted(members.tolist()) == [101, 5000], "sizes 100 and 101 against propose_points = 100: > and not >="
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    logit = dev(logits)
    prob = logit if form == "hip-logit" else torch.softmax(logit, -1)
    run = lambda: pointgroup.proposals(dev(point_cluster), dev(sizes), dev(firsts), dev(segment_pred), prob, 100,  # noqa: E731
                                       is_logit=form == "hip-logit")
    scores, masks, classes = run()
    assert scores.dtype == torch.float32 and masks.dtype == torch.int32 and classes.dtype == torch.int64
    assert np.array_equal(classes.cpu().numpy(), want_classes) and np.array_equal(masks.cpu().numpy(), want_masks)
    rel = np.abs(scores.cpu().numpy().astype(np.float64) - want_scores) / want_scores
    bound = (members + 8) * 2.0 ** -24
    print("pointgroup-scores", form, "relative error", rel, "bound", bound)
    assert (rel <= bound).all()
    if form != "torch":
        again, _, _ = run()
        assert torch.equal(again, scores), "two runs give the same bits"
    # nothing kept: (0,), (0, N), (0,)
    scores, masks, classes = pointgroup.proposals(dev(point_cluster), dev(sizes), dev(firsts), dev(segment_pred), prob, 10 ** 6)
    assert scores.shape == (0,) and masks.shape == (0, n) and classes.shape == (0,)


# ---------------------------------------------------------------------------------------------------------- offset loss ----
def _loss_runs(case):
    """float64 restatement, eager fp32 statements and the HIP path on one input: (l1, cos, grad) each"""
    from ao_amd import pointgroup

    pred, coord, center, instance = C.loss_case(*case[0], **case[1])
    g_l1, g_cos = 0.75, 1.25  # (exact in fp32: the float64 restatement and the device runs get the same upstream scalars)
    f64 = R.bias_loss(pred, coord, center, instance, -1, g_l1, g_cos)
    runs = {}
    for path in ("torch", "hip"):
        p = torch.from_numpy(pred).cuda().requires_grad_(True)
        args = (p, torch.from_numpy(coord).cuda(), torch.from_numpy(center).cuda(), torch.from_numpy(instance).cuda(), -1)
        if path == "torch":
            l1, cos = pointgroup.bias_loss_torch(*args)
        else:
            l1, cos = pointgroup.ops._BiasLoss.apply(*args)
        (g_l1 * l1 + g_cos * cos).backward()
        runs[path] = (float(l1.detach().double()), float(cos.detach().double()), p.grad.double().cpu().numpy())
    return f64, runs, instance


LOSS_CASES = {"n300": ((300, 1), {}), "n5000": ((5000, 2), {}), "all_masked": ((300, 3), dict(all_masked=True))}


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_bias_loss(name):
    f64, runs, instance = _loss_runs(LOSS_CASES[name])
    bad = []
    for k, key in enumerate(("bias_l1_loss", "bias_cosine_loss")):
        eager, ours = abs(runs["torch"][k] - f64[k]), abs(runs["hip"][k] - f64[k])
        allowed = max(2 * eager, 4 * float(np.spacing(np.float32(abs(f64[k])))))
        print("pointgroup-loss %-10s %-16s f64 %+.9e eager err %.3e hip err %.3e allowed %.3e" % (name, key, f64[k], eager, ours, allowed))
        if not ours <= allowed:
            bad.append((key, ours, allowed))
    if name == "all_masked":
        assert runs["hip"][0] == 0.0 and runs["hip"][1] == 0.0 and not runs["hip"][2].any()
        assert f64[0] == 0.0 and f64[1] == 0.0
    else:
        keep, share = C.kept_rows(f64[2], instance)
        print("pointgroup-loss %-10s gradient rows compared: %d of %d used (%.1f %%)" % (name, keep.sum(), (instance != -1).sum(), 100 * share))
        assert share >= 0.9 and keep[3] and keep[5], "the case keeps at least 90 % of the used rows, the zero row and the pred == gt row"
        want = f64[2][keep]
        eager, ours = np.abs(runs["torch"][2][keep] - want), np.abs(runs["hip"][2][keep] - want)
        allowed = np.maximum(2 * eager, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
        print("pointgroup-loss %-10s gradient: largest eager err %.3e hip err %.3e, worst hip / allowed %.3f" % (
            name, eager.max(), ours.max(), (ours / allowed).max()))
        if not (ours <= allowed).all():
            bad.append(("gradient", float((ours / allowed).max())))
        # the rules: ignored rows get 0, sign(0) = 0 where pred == gt, the zero row gets g * gt_norm / 1e-8 from the quotient alone
        assert not runs["hip"][2][instance == -1].any()
        assert np.isfinite(runs["hip"][2]).all()
    assert not bad, bad


def test_bias_loss_zero_row_with_an_ordinary_target():
    """a zero bias_pred row whose target is of ordinary size: its gradient g * gt_norm / 1e-8 / count dwarfs every other row's"""
    pred, coord, center, instance = C.loss_case(300, 4, special=False)
    instance[7], pred[7] = 2, 0.0
    f64 = R.bias_loss(pred, coord, center, instance, -1)
    from ao_amd import pointgroup

    grads = {}
    for path in ("torch", "hip"):
        p = torch.from_numpy(pred).cuda().requires_grad_(True)
        args = (p, torch.from_numpy(coord).cuda(), torch.from_numpy(center).cuda(), torch.from_numpy(instance).cuda(), -1)
        l1, cos = pointgroup.bias_loss_torch(*args) if path == "torch" else pointgroup.ops._BiasLoss.apply(*args)
        (l1 + cos).backward()
        grads[path] = p.grad[7].double().cpu().numpy()
    want = f64[2][7]
    assert np.abs(want).max() > 1e4
    eager, ours = np.abs(grads["torch"] - want), np.abs(grads["hip"] - want)
    allowed = np.maximum(2 * eager, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    print("pointgroup-loss zero row: f64", want, "eager err", eager, "hip err", ours)
    assert (ours <= allowed).all()


def test_bias_loss_under_autocast_is_fp32(monkeypatch):
    from ao_amd import pointgroup

    pred, coord, center, instance = (torch.from_numpy(v).cuda() for v in C.loss_case(300, 1))
    plain = pointgroup.bias_loss(pred, coord, center, instance, -1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = pointgroup.bias_loss(pred.bfloat16().float(), coord, center, instance, -1)
        same = pointgroup.bias_loss(pred, coord, center, instance, -1)
    assert same[0].dtype == torch.float32 and torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1])
    assert cast[0].dtype == torch.float32
    monkeypatch.setenv("AO_AMD_PG", "torch")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        eager = pointgroup.bias_loss(pred, coord, center, instance, -1)
    assert eager[0].dtype == torch.float32 and abs(float(eager[0]) - float(plain[0])) <= 1e-5 * abs(float(plain[0]))
