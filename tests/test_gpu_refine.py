"""GPU: REAL's epoch-end label refinement (ao_amd/ptv2/refine.py on ao_amd/csrc/refine.hip).

Everything but the confidence is integer or a choice, and the inputs are built so that the reference's choices do not hang on
a rounding (tests/refine_cases.py: `rivals`, checked on the CPU by tests/test_refine_host.py): pred, the prompts in order, the
votes, the labels and the count must EQUAL tests/golden/refine.npz (the reference's own statements) for the two fixture rooms,
and tests/refine_ref.py (pinned to that fixture on the CPU) for the small shapes.  The confidence is held to twice
`conf_spread` against a float64 softmax margin: conf_spread is the distance of the reference's own fp32 confidence from float64
on the fixture's rows, recorded when the fixture was made (3.2e-7).  Both paths run: HIP and AO_AMD_REFINE=torch.
"""
import warnings

import numpy as np
import pytest
import torch

from tests import refine_cases as RC
from tests import refine_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = ["hip", "torch"]


@pytest.fixture(scope="module")
def fx():
    return RC.load()


@pytest.fixture(scope="module")
def conf_bound(fx):
    return 2 * max(float(fx[tag + "_conf_spread"]) for tag in RC.CASES)


def use(path, monkeypatch):
    if path == "torch":
        monkeypatch.setenv("AO_AMD_REFINE", "torch")
    else:
        monkeypatch.delenv("AO_AMD_REFINE", raising=False)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def seeded_masks(case):
    return lambda view, uv, k: dev(RC.masks_for(case, view, uv.cpu().numpy(), k.cpu().numpy()))


def run_scene(case, masks_for=None):
    """refine_scene on the case's host arrays; every output as numpy"""
    from ao_amd.ptv2 import refine_scene

    d = {}
    label, updated, touched = refine_scene(case["logits"], case["coord"], case["label"], case["present"],
                                           [(b, v) for v, b in enumerate(case["bridges"])], masks_for or seeded_masks(case), details=d)
    assert isinstance(label, np.ndarray) and label.shape == case["label"].shape and label.dtype == case["label"].dtype
    out = {k: v.cpu().numpy() for k, v in d.items() if k != "seen"}
    out.update(label=label.reshape(-1), updated=updated, touched=touched, seen=d["seen"])
    return out


def same_as_reference(out, ref, conf_bound, logits):
    assert np.array_equal(out["pred"], ref["pred"])
    conf64 = RR.confidence(logits, np.float64)[1]
    err = float(np.abs(out["conf"].astype(np.float64) - conf64).max()) if conf64.size else 0.0
    print("conf: max |device - float64| = %.3e (bound %.3e)" % (err, conf_bound))
    assert err <= conf_bound
    assert np.array_equal(out["prompt_idx"], ref["prompt_idx"]) and np.array_equal(out["prompt_cls"], ref["prompt_cls"])
    assert list(out["seen"]) == list(ref["seen"])
    assert np.array_equal(out["vote"], ref["vote"])
    assert np.array_equal(out["label"], np.asarray(ref["label"]).reshape(-1))
    assert out["updated"] == int(ref["updated"]) and out["touched"] == bool(ref["touched"])


# ---- the two fixture rooms end to end ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tag", sorted(RC.CASES))
def test_fixture_scene(fx, conf_bound, tag, path, monkeypatch):
    use(path, monkeypatch)
    case = RC.room(tag)
    out = run_scene(case)
    same_as_reference(out, {k: fx["%s_%s" % (tag, k)] for k in ("pred", "prompt_idx", "prompt_cls", "seen", "vote", "label",
                                                                "updated", "touched")}, conf_bound, case["logits"])
    assert out["seen"][-1] == 0 and out["touched"]  # the last view sees points but no prompt


def test_two_runs_give_identical_outputs(monkeypatch):
    use("hip", monkeypatch)
    case = RC.room("c13")
    a, b = run_scene(case), run_scene(case)
    for k in ("pred", "conf", "prompt_idx", "prompt_cls", "vote", "label"):
        assert np.array_equal(a[k], b[k]), k
    assert a["updated"] == b["updated"]


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("c", [2, 13, 20])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_confidence(conf_bound, n, c, path, monkeypatch):
    from ao_amd.ptv2 import scene_confidence

    use(path, monkeypatch)
    rng = np.random.default_rng(100 * n + c)
    logits = rng.integers(-24, 25, (n, c)).astype(np.float32) / 4
    if n > 8:
        logits[1] = 0.0                          # every class maximal: the first, margin 0
        logits[2] = -100.0                       # unseen: -1, uniform, margin 0
        logits[3, [1, c - 1]] = 7.0              # c > 2: two equal maxima, the first of them, margin 0
        logits[4, 0], logits[4, 1:] = -100.0, 1  # unseen by the reference's test, whatever the other columns say
    pred, conf = scene_confidence(dev(logits))
    assert pred.dtype == torch.int32 and conf.dtype == torch.float32 and pred.shape == conf.shape == (n,)
    want, _ = RR.confidence(logits)
    conf64 = RR.confidence(logits, np.float64)[1]
    assert np.array_equal(pred.cpu().numpy(), want)
    assert float(np.abs(conf.cpu().numpy().astype(np.float64) - conf64).max()) <= conf_bound
    if n > 8:
        assert pred[1:5].tolist() == [0, -1, 1, -1] and conf[1:3].tolist() == [0.0, 0.0] and (c == 2 or float(conf[3]) == 0.0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("c", [2, 13])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_rooms(conf_bound, n, c, path, monkeypatch):
    use(path, monkeypatch)
    case = RC.make_room("small", 7 * n + c, n, c, 3.2, 2.7, absent=(1,) if c > 2 else (), flat=(2.0, 9.5, 12.0))
    ref = RR.refine_scene(case["logits"], case["coord"], case["label"], case["present"],
                          [(b, v) for v, b in enumerate(case["bridges"])], lambda v, uv, k: RC.masks_for(case, v, uv, k))
    same_as_reference(run_scene(case), ref, conf_bound, case["logits"])
    assert n == 1 or ref["prompt_idx"].size > 0


# ---- cells -----------------------------------------------------------------------------------------------------------------------------

def sharp_logits(n, c, cls, base=8.0):
    """row i predicts cls[i] with a confidence near 1, a different one for every row"""
    logits = np.zeros((n, c), np.float32)
    logits[np.arange(n), cls] = base + 0.25 * np.arange(n)
    return logits


def prompts_of(coord, logits, label, present, bounds=None):
    from ao_amd.ptv2 import grid_prompts, scene_confidence

    pred, conf = scene_confidence(dev(logits))
    idx, cls = grid_prompts(dev(coord), pred, conf, dev(label, torch.int32), dev(present), bounds=bounds)
    p, f = pred.cpu().numpy(), conf.cpu().numpy()
    want = RR.prompts(coord, p, f, label, present)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(cls.cpu().numpy(), want[1])
    return idx.tolist(), cls.tolist()


@pytest.mark.parametrize("path", PATHS)
def test_cell_boundaries(path, monkeypatch):
    use(path, monkeypatch)
    coord = np.array([[1.0, 2.0, 0], [1.25, 0.0, 0], [1.5, 2.25, 0], [1.75, 2.5, 0], [1.75, 2.25, 0], [4.2, 2.4, 0],
                      [2.2, 2.7, 0], [2.2, 2.45, 0]], np.float32)
    # 0: x == min_x (min_x = 1.0)   1: y == min_y   2: x on min + 1 * 0.5   3: y on min + 5 * 0.5, which is also the end of the
    # last y cell (Ly = 2.7 -> ny = 5)   4: cell (1, 4)   5: x = max, in cell 6 of nx = 8 (Lx = 3.2: the cells run to 5.0)
    # 6: the y strip beyond ny * 0.5 = 2.5   7: cell (2, 4)
    n = coord.shape[0]
    logits, label, present = sharp_logits(n, 2, np.ones(n, np.int64)), np.zeros(n, np.int64), np.ones(2, np.uint8)
    for bounds in (None, (1.0, np.float32(4.2), 0.0, np.float32(2.7))):
        assert prompts_of(coord, logits, label, present, bounds) == ([4, 7, 5], [1, 1, 1])
    # every point of one cell, three classes: one prompt per class, ascending
    coord = np.array([[0, 0, 0], [3.2, 2.7, 0], [0.3, 0.3, 0], [0.31, 0.3, 0], [0.32, 0.3, 0], [0.33, 0.3, 0]], np.float32)
    logits = sharp_logits(6, 3, np.array([0, 0, 2, 1, 0, 2]))
    assert prompts_of(coord, logits, np.full(6, 1), np.ones(3, np.uint8)) == ([4, 5], [0, 2])  # 3: label == pred; 5 beats 2


@pytest.mark.parametrize("path", PATHS)
def test_rooms_without_prompts(path, monkeypatch):
    from ao_amd.ptv2 import LabelRefiner

    use(path, monkeypatch)
    case = RC.make_room("flat", 3, 65, 13, 3.2, 2.7)
    pred = RR.confidence(case["logits"])[0]
    label = case["label"].reshape(-1)

    def never(pixel_xy, prompt_cls):
        raise AssertionError("masks_for was called without a visible prompt")

    low = case["coord"].copy()
    low[:, 1] *= 0.4 / 2.7                                   # Ly < 0.5: ny == 0
    unseen = np.full_like(case["logits"], -100.0)
    absent = np.zeros(13, np.uint8)
    for coord, logits, lab, present in ((low, case["logits"], label, case["present"]),
                                        (case["coord"], unseen, label, case["present"]),
                                        (case["coord"], case["logits"], pred, case["present"]),   # label == pred everywhere
                                        (case["coord"], case["logits"], label, absent)):          # no class is present
        r = LabelRefiner(13).begin(dev(logits), dev(coord), dev(lab, torch.int32), dev(present))
        assert r.prompt_idx.numel() == 0 and r.prompt_cls.numel() == 0
        assert r.vote_view(dev(case["bridges"][0]), never) == 0
        out, updated, touched = r.finish()
        assert np.array_equal(out.cpu().numpy(), lab) and updated == 0 and touched is False
    # one absent class takes only its own prompts away
    full = RR.prompts(case["coord"], *RR.confidence(case["logits"]), label, np.ones(13, np.uint8))
    some = np.ones(13, np.uint8)
    some[full[1][0]] = 0
    idx, cls = prompts_of(case["coord"], case["logits"], label, some)
    assert cls and full[1][0] not in cls and idx == [i for i, k in zip(*full) if k != full[1][0]]


@pytest.mark.parametrize("path", PATHS)
def test_equal_confidence_lowest_index_wins(path, monkeypatch):
    use(path, monkeypatch)
    coord = np.array([[0, 0, 0], [3.2, 2.7, 0]] + [[0.3 + 0.002 * i, 0.3, 0] for i in range(70)], np.float32)
    cls = np.zeros(72, np.int64)
    logits = sharp_logits(72, 2, cls, base=3.0)
    logits[2:] = 0.0
    logits[2:, 0] = 5.0        # 70 identical rows in cell (0, 0) ...
    logits[[9, 40, 71], 0] = 9.0  # ... three sharper identical rows among them: 9 is the lowest
    assert prompts_of(coord, logits, np.ones(72, np.int64), np.ones(2, np.uint8)) == ([9], [0])
    logits[9, 0] = 5.0
    assert prompts_of(coord, logits, np.ones(72, np.int64), np.ones(2, np.uint8)) == ([40], [0])


# ---- votes -----------------------------------------------------------------------------------------------------------------------------

def dense_view_case(seed=5, n=130, c=3, height=4, width=5):
    """a small room whose views put many points on every pixel, pixel 0 and element [0][0] included; dense random masks"""
    case = RC.make_room("dense", seed, n, c, 3.2, 2.7, flat=(2.0, 9.5, 12.0), height=height, width=width)
    rng = np.random.default_rng(seed)
    case["bridges"] = [np.stack([rng.integers(0, height + 1, n), rng.integers(0, width + 1, n), rng.random(n) < 0.8], 1).astype(np.int64)
                       for _ in range(3)]

    def masks(view, uv, k):
        m = np.random.default_rng([seed, view]).random((len(k), height, width)) < 0.5
        m[:, 0, 0] = True
        return m

    return case, masks


@pytest.mark.parametrize("path", PATHS)
def test_vote_semantics(conf_bound, path, monkeypatch):
    use(path, monkeypatch)
    case, masks = dense_view_case()
    ref = RR.refine_scene(case["logits"], case["coord"], case["label"], case["present"],
                          [(b, v) for v, b in enumerate(case["bridges"])], masks)
    # what the inputs exercise, by the restatement: index -1 in both axes, the cleared element, tied modes (the smallest class
    # wins), modes that are not the prompt's class (no vote), prompts a view does not see
    tied = other = 0
    for v, bridge in enumerate(case["bridges"]):
        seen = np.nonzero(bridge[ref["prompt_idx"], 2] == 1)[0]
        assert 0 < seen.size < ref["prompt_idx"].size
        rows, inside = RR.inside_points(bridge, masks(v, None, seen))
        assert (bridge[rows, 0] == 0).any() and (bridge[rows, 1] == 0).any() and ((bridge[rows, 0] == 1) & (bridge[rows, 1] == 1)).any()
        assert not inside[:, (bridge[rows, 0] == 1) & (bridge[rows, 1] == 1)].any()
        for p in range(seen.size):
            hist = np.bincount(ref["pred"][rows][inside[p] & (ref["conf"][rows] > 0.9)], minlength=3)
            tied += hist.max() > 0 and (hist == hist.max()).sum() > 1 and np.argmax(hist) == ref["prompt_cls"][seen[p]]
            other += hist.max() > 0 and np.argmax(hist) != ref["prompt_cls"][seen[p]]
    assert tied > 0 and other > 0 and ref["vote"].max() >= 2
    same_as_reference(run_scene(case, lambda view, uv, k: dev(masks(view, uv, k))), ref, conf_bound, case["logits"])


@pytest.mark.parametrize("path", PATHS)
def test_masks_for_gets_the_visible_prompts(path, monkeypatch):
    from ao_amd.ptv2 import LabelRefiner

    use(path, monkeypatch)
    case, masks = dense_view_case()
    r = LabelRefiner(3).begin(dev(case["logits"]), dev(case["coord"]), dev(case["label"].reshape(-1), torch.int32), dev(case["present"]))
    idx, cls = r.prompt_idx.cpu().numpy(), r.prompt_cls.cpu().numpy()
    bridge = case["bridges"][0]
    seen = np.nonzero(bridge[idx, 2] == 1)[0]
    got = {}

    def masks_for(pixel_xy, prompt_cls):
        got.update(xy=pixel_xy, cls=prompt_cls)
        return dev(masks(0, None, seen)).to(torch.uint8)  # uint8 as well as bool

    assert r.vote_view(dev(bridge), masks_for) == seen.size  # an int64 bridge
    assert got["xy"].dtype == torch.float32 and got["xy"].is_cuda and got["cls"].dtype == torch.int32
    assert np.array_equal(got["xy"].cpu().numpy(), bridge[idx[seen], :2].astype(np.float32))
    assert np.array_equal(got["cls"].cpu().numpy(), cls[seen])
    with pytest.raises(ValueError, match="masks_for returned"):
        r.vote_view(dev(bridge), lambda xy, k: torch.zeros((1, 4, 5), dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("path", PATHS)
def test_pixel_outside_the_image_raises_index_error(path, monkeypatch):
    """the bounds guard: u = H + 1 on a visible point is skipped and reported, nothing is read outside the masks"""
    from ao_amd.ptv2 import LabelRefiner

    use(path, monkeypatch)
    case, masks = dense_view_case()
    args = (dev(case["logits"]), dev(case["coord"]), dev(case["label"].reshape(-1), torch.int32), dev(case["present"]))
    r = LabelRefiner(3).begin(*args)
    idx = r.prompt_idx.cpu().numpy()
    bridge = case["bridges"][0].copy()
    victim = [i for i in np.nonzero(bridge[:, 2] == 1)[0] if i not in set(idx.tolist())][0]
    skipped = bridge.copy()
    skipped[victim, 2] = 0
    bridge[victim, 0] = 4 + 1
    seen = np.nonzero(bridge[idx, 2] == 1)[0]
    serve = lambda xy, k: dev(masks(0, None, seen))  # noqa: E731
    r.vote_view(dev(bridge), serve)
    with pytest.raises(IndexError, match="pixel"):
        r.finish()
    torch.cuda.synchronize()
    clean = LabelRefiner(3).begin(*args)
    clean.vote_view(dev(skipped), serve)
    assert torch.equal(r.vote, clean.vote) and int(clean.vote.sum()) > 0  # every other point voted as if the bad one were unseen
    clean.finish()


# ---- update ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n,c", [(1, 2), (65, 13), (300, 20)])
def test_update(n, c, path, monkeypatch):
    from ao_amd.ptv2 import LabelRefiner

    use(path, monkeypatch)
    case = RC.make_room("upd", n + c, n, c, 3.2, 2.7)
    rng = np.random.default_rng(n)
    label = case["label"].reshape(-1)
    r = LabelRefiner(c).begin(dev(case["logits"]), dev(case["coord"]), dev(label, torch.int32), dev(case["present"]))
    pred = r.pred.cpu().numpy()
    vote = rng.integers(0, 3, (n, c)).astype(np.int32) * (rng.random((n, 1)) < 0.8)   # ties between classes, rows without a vote
    agree = rng.random(n) < 0.5
    vote[agree, np.clip(pred[agree], 0, c - 1)] += 3                                   # ... rows whose result is the prediction
    if n > 8:
        vote[5] = 0
        vote[5, [np.clip(pred[5], 0, c - 2), c - 1]] = 2                              # a tie: the first maximal class
    r.vote.copy_(dev(vote))
    r.touched = True
    out, updated, touched = r.finish()
    want, count = RR.update(vote, pred, label)
    assert np.array_equal(out.cpu().numpy(), want) and updated == count and touched
    result = np.argmax(vote, 1)
    keep = (vote.sum(1) == 0) | (result != pred) | (pred == -1)
    assert np.array_equal(want[keep], label[keep]) and (n == 1 or (0 < keep.sum() < n and count > 0))


# ---- streams and synchronisation ---------------------------------------------------------------------------------------------------------

def test_current_stream_and_host_reads(fx, monkeypatch):
    """everything is enqueued on the current stream; `begin` (with the bounds given) and `vote_view` read once each, the
    confidence pass and finish(check=False) not at all"""
    from ao_amd.ptv2 import LabelRefiner, scene_confidence

    use("hip", monkeypatch)
    case = RC.room("c13")
    logits, coord, present = dev(case["logits"]), dev(case["coord"]), dev(case["present"])
    label = dev(case["label"].reshape(-1), torch.int32)
    bridges = [dev(b, torch.int32) for b in case["bridges"]]
    lo, hi = case["coord"].min(0), case["coord"].max(0)
    bounds = (lo[0], hi[0], lo[1], hi[1])
    idx = fx["c13_prompt_idx"]
    served = [dev(RC.masks_for(case, v, b[idx][b[idx, 2] == 1][:, :2], fx["c13_prompt_cls"][b[idx, 2] == 1]))
              for v, b in enumerate(case["bridges"])]
    LabelRefiner(13).begin(logits, coord, label, present, bounds).vote_view(bridges[0], lambda xy, k: served[0])  # warm
    torch.cuda.synchronize()

    def reads(fn):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return out, len([w for w in seen if "called a synchronizing" in str(w.message)])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, count = reads(lambda: scene_confidence(logits))
        assert count == 0
        r, count = reads(lambda: LabelRefiner(13).begin(logits, coord, label, present, bounds))
        assert count == 1
        for v, bridge in enumerate(bridges):
            _, count = reads(lambda: r.vote_view(bridge, lambda xy, k: served[v]))
            assert count == 1
        (out, updated, touched), count = reads(lambda: r.finish(check=False))
        assert count == 0 and torch.is_tensor(updated) and updated.is_cuda and touched
    side.synchronize()
    assert np.array_equal(r.vote.cpu().numpy(), fx["c13_vote"]) and np.array_equal(out.cpu().numpy(), fx["c13_label"])
    assert int(updated) == int(fx["c13_updated"])
