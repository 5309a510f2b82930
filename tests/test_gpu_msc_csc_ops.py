"""GPU: ao_amd.msc.csc_nce (ao_amd/csrc/msc_csc.hip), the partitioned InfoNCE loss of MSC-v1m2, against the float64 restatement
tests/msc_csc_ref.py, on both paths (HIP and AO_AMD_MSC=torch).

The project's M-rule (DESIGN.md sections 2, 13, 16): the kernel's error against float64 is at most M_TOL * max(the error of the
reference's eager fp32 statements on the same GPU, 2^-24), relative error for the three scalars and relative L2 for the two
gradients.  Where no scene has more than two pairs a relative error is taken against the larger of the value and the term that
is subtracted in it (section 13's convention: at M = 1 the log-sum-exps and the positive term cancel to an exact zero, of which
no fp32 evaluation has a relative error).  M_TOL (tests/msc_csc_cases.py): twice the worst ratio measured on an MI355X over the
cases below, rounded up to a power of two, at least 1 and at most 64; DESIGN.md section 16 tables the ratios."""
import numpy as np
import pytest
import torch

from tests import msc_csc_ref as C
from tests.msc_csc_cases import FLOOR, KEYS, M_TOL, csc_case

pytestmark = pytest.mark.gpu

SIZES = [((1,), 96), ((2,), 96), ((63,), 96), ((64,), 96), ((65,), 96), ((257,), 96), ((1000,), 96), ((64, 0, 65), 96),
         ((65, 64), 4), ((65, 64), 32), ((65, 64), 256)]
GEOMETRY = {"room": {}, "big_room": dict(geometry="big"), "equal_z": dict(special="equal_z"), "identical": dict(special="identical"),
            "r1_above_r2": dict(r=(0.5, 0.125))}
FEATURES = ["dup1", "dup2", "zero_row", "scale_1e3", "scale_1e-3"]
_REF = {}


def reference(key, case, t):
    """the float64 values of a case, computed once"""
    if (key, t) not in _REF:
        _REF[key, t] = C.csc_nce(case["f1"], case["f2"], case["o1"], case["o2"], case["offset1"], case["pairs"], t, case["r1"],
                                 case["r2"], g=1.7)
    return _REF[key, t]


def run(case, t, g=1.7, partitions=4):
    from ao_amd import msc

    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    x1, x2 = dev(case["f1"]).requires_grad_(True), dev(case["f2"]).requires_grad_(True)
    loss, pos_sim, neg_sim = msc.csc_nce(x1, x2, dev(case["o1"]), dev(case["o2"]), dev(case["offset1"]), dev(case["pairs"]), t,
                                         case["r1"], case["r2"], partitions)
    assert not pos_sim.requires_grad and not neg_sim.requires_grad and loss.dtype == torch.float32
    (loss * g).backward()
    return dict(loss=loss.detach().cpu().numpy(), pos_sim=pos_sim.cpu().numpy(), neg_sim=neg_sim.cpu().numpy(),
                df1=x1.grad.cpu().numpy(), df2=x2.grad.cpu().numpy())


def errors(got, ref, small):
    scale = dict.fromkeys(KEYS, 0.0)
    if small:
        scale.update(loss=abs(ref["loss_pos"]), neg_sim=abs(ref["neg_sub"]), df1=np.linalg.norm(ref["df1_pos"]),
                     df2=np.linalg.norm(ref["df2_pos"]))
    return {k: float(np.linalg.norm(np.asarray(got[k], np.float64) - ref[k]) / max(np.linalg.norm(ref[k]), scale[k])) for k in KEYS}


def check(name, counts, c, t, monkeypatch, **kwargs):
    case = csc_case(counts, c=c, seed=1000 + 7 * sum(counts) + c, **kwargs)
    ref = reference((name, counts, c), case, t)
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    got = run(case, t)
    monkeypatch.setenv("AO_AMD_MSC", "torch")
    eager = run(case, t)
    small = max(counts) <= 2
    e_kernel, e_eager = errors(got, ref, small), errors(eager, ref, small)
    for k in KEYS:
        print("msc csc_nce %-11s M %-12s C %3d t %.2f %-7s kernel %.3e eager %.3e ratio %.2f" % (
            name, counts, c, t, k, e_kernel[k], e_eager[k], e_kernel[k] / max(e_eager[k], FLOOR)))
    for k in KEYS:
        assert e_kernel[k] <= M_TOL[k] * max(e_eager[k], FLOOR), (name, counts, c, t, k, e_kernel[k], e_eager[k])
    # rows that no pair names: exactly zero
    unnamed1 = np.setdiff1d(np.arange(len(case["f1"])), case["pairs"][:, 0])
    unnamed2 = np.setdiff1d(np.arange(len(case["f2"])), case["pairs"][:, 1])
    assert len(unnamed1) >= 5 and len(unnamed2) >= 3
    assert not got["df1"][unnamed1].any() and not got["df2"][unnamed2].any()
    assert np.isfinite(got["df1"]).all() and np.isfinite(got["df2"]).all()
    return case


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("counts,c", SIZES)
def test_csc_nce_sizes(counts, c, t, monkeypatch):
    check("plain", counts, c, t, monkeypatch)


@pytest.mark.parametrize("t", [0.4, 0.07])
def test_csc_nce_interleaved_scenes(t, monkeypatch):
    """the pairs of two scenes in a random order, as the max_pair permutation leaves them"""
    case = check("interleaved", (130, 70), 96, t, monkeypatch, interleave=True)
    scene = C.scenes_of(case["pairs"], case["offset1"], len(case["o1"]))
    assert (np.diff(scene) < 0).sum() > 20


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_csc_nce_geometry(name, t, monkeypatch):
    case = check(name, (65, 64), 96, t, monkeypatch, **GEOMETRY[name])
    total = sum(c.sum(0) for c in C.class_counts(case["o1"], case["o2"], case["offset1"], case["pairs"], case["r1"], case["r2"]))
    if name in ("room", "equal_z", "identical"):
        assert (total > 0).all(), "all five classes"
    if name == "big_room":
        assert total[0] > 0 and total[1] > 0 and total[2] == total[3] == 0
    if name == "r1_above_r2":
        assert total[0] == total[1] == 0 and total[2] > 0 and total[3] > 0
    if name == "equal_z":
        assert total[4] >= 2 * 90, "ten pairs on one z: ninety off-diagonal elements with rel_z == 0 in either scene"


@pytest.mark.parametrize("t", [0.4, 0.07])
@pytest.mark.parametrize("name", FEATURES)
def test_csc_nce_special_rows(name, t, monkeypatch):
    check(name, (65, 64), 96, t, monkeypatch, special=name)


@pytest.mark.parametrize("name", ["room", "big_room", "equal_z"])
def test_class_counts_pin_the_partition(name, monkeypatch):
    """Every feature row the same vector: S is one constant, lse_k - S_ii / t = log(1 + n_ki), and the loss is a function of the
    integer class counts per row alone.  A transposed rel, a wrong override order or a wrong rel_z == 0 rule changes counts.
    Bound: moving ONE element to another class changes a scene's term by about 1 / (M n) ~ 5e-4 of ~8, a relative 6e-5; the fp32
    evaluation of log(sum) + (1 - S_ii) / t, two numbers of the size of log M, stays near 1e-7 (a form that subtracts two numbers
    near 1 / t reaches 1e-6 at t = 0.07).  1e-5 separates the two."""
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    case = csc_case((65, 64), c=96, seed=31, **GEOMETRY[name])
    row = np.random.default_rng(3).normal(0.5, 1.0, 96).astype(np.float32)
    case["f1"], case["f2"] = np.tile(row, (len(case["f1"]), 1)), np.tile(row, (len(case["f2"]), 1))
    counts = C.class_counts(case["o1"], case["o2"], case["offset1"], case["pairs"], case["r1"], case["r2"])
    assert [len(c) for c in counts] == [65, 64] and all((c.sum(1) == len(c) - 1).all() for c in counts)
    want = C.loss_of_counts(counts, 2)
    for t in (0.4, 0.07):
        got = run(case, t)
        print("msc csc_nce class counts %-8s t %.2f loss %.9g from counts %.9g rel %.2e" % (
            name, t, float(got["loss"]), want, abs(float(got["loss"]) - want) / want))
        assert abs(float(got["loss"]) - want) <= 1e-5 * want
    # the transposed partition (rel = x_i - y_j) has other counts: the pin can tell
    swapped = C.class_counts(case["o2"], case["o1"], case["offset2"], case["pairs"][:, ::-1], case["r1"], case["r2"])
    if name != "big_room":
        assert abs(C.loss_of_counts(swapped, 2) - want) > 1e-4 * want


def test_csc_nce_same_bits_twice(monkeypatch):
    monkeypatch.setenv("AO_AMD_MSC", "hip")
    for counts, kwargs, t in (((65, 64), dict(special="dup2"), 0.4), ((130, 70), dict(interleave=True), 0.07), ((1000,), {}, 0.4)):
        case = csc_case(counts, seed=5, **kwargs)
        first, again = run(case, t), run(case, t)
        for k in first:
            assert np.array_equal(first[k], again[k]), (counts, k)


def test_csc_nce_outside_the_limits(monkeypatch):
    """C = 6 is no multiple of 4 and t = 0.02 is below 1 / CSC_MAX_INV_T: the eager statements run, whatever the switch says;
    no pair at all raises; a pair outside its operand turns the outputs NaN without a fault and leaves no gradient"""
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    for c, t in ((6, 0.4), (96, 0.02)):
        case = csc_case((65, 64), c=c, seed=9)
        got = run(case, t)
        x1, x2 = dev(case["f1"]).requires_grad_(True), dev(case["f2"]).requires_grad_(True)
        loss, pos_sim, neg_sim = msc.csc_nce_torch(x1, x2, dev(case["o1"]), dev(case["o2"]), dev(case["offset1"]), dev(case["pairs"]),
                                                   t, case["r1"], case["r2"], 4)
        (loss * 1.7).backward()
        assert np.array_equal(got["loss"], loss.detach().cpu().numpy()) and np.array_equal(got["df1"], x1.grad.cpu().numpy())
        assert np.array_equal(got["pos_sim"], pos_sim.cpu().numpy()) and np.array_equal(got["neg_sim"], neg_sim.cpu().numpy())
        assert np.array_equal(got["df2"], x2.grad.cpu().numpy())
    args = (dev(case["o1"]), dev(case["o2"]), dev(case["offset1"]))
    with pytest.raises(ValueError, match="no pair"):
        msc.csc_nce(x1, x2, *args, torch.zeros((0, 2), dtype=torch.int64, device="cuda"), 0.4, 0.125, 0.5)
    for column, bad in ((1, len(case["f2"])), (0, len(case["f1"])), (0, -1)):
        pairs = case["pairs"].copy()
        pairs[4, column] = bad
        x1 = dev(case["f1"]).requires_grad_(True)
        out = msc.csc_nce(x1, dev(case["f2"]), *args, dev(pairs), 0.4, 0.125, 0.5)
        assert all(bool(torch.isnan(v)) for v in out)
        out[0].backward()
        assert bool(torch.isfinite(x1.grad).all()), "the backward reads nothing outside either"


def test_csc_nce_under_autocast_and_partitions(monkeypatch):
    from ao_amd import msc

    monkeypatch.setenv("AO_AMD_MSC", "hip")
    case = csc_case((65, 64), c=32, seed=3)
    want = run(case, 0.4)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, _, _ = msc.csc_nce(dev(case["f1"]), dev(case["f2"]), dev(case["o1"]), dev(case["o2"]), dev(case["offset1"]),
                                 dev(case["pairs"]), 0.4, case["r1"], case["r2"])
    assert loss.dtype == torch.float32 and np.array_equal(loss.cpu().numpy(), want["loss"])
    # partitions only divides
    two = run(case, 0.4, partitions=2)
    assert abs(float(two["loss"]) - 2 * float(want["loss"])) <= 2.0 ** -22 * float(two["loss"])
    assert np.array_equal(two["pos_sim"], want["pos_sim"]) and np.array_equal(two["neg_sim"], want["neg_sim"])


def test_no_m_by_m_tensor(monkeypatch):
    """One scene, M = n1 = n2 = 4096, C = 96, forward and backward: the allocator's peak rises by at most 16 MB, a quarter of one
    fp32 `sim` (the kernels keep about ten (M, C) arrays and 11 floats per pair), where the eager statements hold several whole
    (M, M) arrays.  A condition, not a measurement."""
    from ao_amd import msc

    m, c = 4096, 96
    g = torch.Generator(device="cuda").manual_seed(7)
    x1 = torch.randn(m, c, device="cuda", generator=g).requires_grad_(True)
    x2 = (0.6 * x1.detach() + 0.4 * torch.randn(m, c, device="cuda", generator=g)).requires_grad_(True)
    o1 = torch.randint(0, 64, (m, 3), device="cuda", generator=g).float() * 2.0 ** -6
    o2 = o1 + torch.randint(-3, 4, (m, 3), device="cuda", generator=g).float() * 2.0 ** -10
    offset = torch.tensor([m], dtype=torch.int32, device="cuda")
    index = torch.stack([torch.randperm(m, device="cuda", generator=g)] * 2, 1)

    def rise(path):
        monkeypatch.setenv("AO_AMD_MSC", path)
        x1.grad = x2.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, _, _ = msc.csc_nce(x1, x2, o1, o2, offset, index, 0.4, 0.125, 0.5)
        loss.backward()
        torch.cuda.synchronize()
        assert x1.grad is not None and bool(torch.isfinite(loss))
        return torch.cuda.max_memory_allocated() - before

    hip, eager = rise("hip"), rise("torch")
    print("msc csc_nce M 4096 C 96: allocator peak rises by %.1f MB (HIP), %.1f MB (eager)" % (hip / 2 ** 20, eager / 2 ** 20))
    assert hip <= 16 << 20
    assert eager > 64 << 20
