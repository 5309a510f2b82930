"""GPU: ao_amd.stratified (ao_amd/csrc/stratified.hip) against tests/st_ref.py.

Exact: the window cells, the pair lists (as sets per row, with offsets and n_max), the transposed lists (a permutation of the
pairs, ascending by pair within a key) and the relative-position index, each against the eager fp32 statements on the same GPU.

Against float64: the three pointops2 operators and window_attention on its three paths.  Every output and every gradient is
compared, the tables' included, and the compared key set is asserted.  The bound is the rule of tests/test_gpu_ptv1_layer.py:
e_kernel <= M[key] * max(e_eager, 2^-24), e_eager the distance from float64 of the fp32 run of st_ref on the same device and
inputs, in relative L2 (and for forward outputs also the largest element error over the largest reference element).  M per key:
twice the worst ratio measured on the MI355X over every case and path, rounded up to a power of two.

Repeatability: two fused runs give the same bits for out, grad_q, grad_k and grad_v.  Memory: a fused forward + backward
allocates a small fraction of one (M, h) fp32 array."""
import numpy as np
import pytest
import torch

from tests import st_cases as SC
from tests import st_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
ATTN_KEYS = {"out", "g_q", "g_k", "g_v", "g_table_q", "g_table_k", "g_table_v"}
FWD_KEYS = {"out"}
# M per key: 2 x the worst e_kernel / e_eager over every case and path, as a power of two
M = {"out": 8, "g_q": 8, "g_k": 8, "g_v": 4, "g_table_q": 4, "g_table_k": 8, "g_table_v": 4, "g_attn": 4}

_REF = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_pairs(name, shifted):
    """the mask-built lists of st_ref on the device, once per (case, shift)"""
    key = ("pairs", name, shifted)
    if key not in _REF:
        c = SC.case(name)
        i0, i1 = R.pair_lists(_dev(c.coords), _dev(c.offset), _dev(c.down_idx), SC.WINDOW, shifted)
        off, n_max = R.csr_of(i0, len(c.coords))
        _REF[key] = (i0, i1, off, n_max)
    return _REF[key]


def our_pairs(name, shifted):
    from ao_amd import stratified

    key = ("ours", name, shifted)
    if key not in _REF:
        c = SC.case(name)
        _REF[key] = stratified.build_pairs(_dev(c.coords), _dev(c.offset), _dev(c.down_idx), SC.WINDOW, shifted)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------- exact ----
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", SC.NAMES)
def test_cells_equal_the_eager_statements(name, shifted):
    from ao_amd import stratified

    c = SC.case(name)
    coords = _dev(c.coords)
    start = coords.min(0).values
    for size in (SC.WINDOW, float(np.float32(SC.WINDOW) * np.float32(2))):
        cell, wcoord = stratified.cells(coords, start, size, shifted)
        want_cell, want_wcoord = R.cells_eager(coords, start, size, shifted)
        assert torch.equal(cell.long(), want_cell), (name, shifted, size)
        assert torch.equal(wcoord.long(), want_wcoord), (name, shifted, size)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", SC.NAMES)
def test_build_pairs_equals_the_mask_statements(name, shifted):
    i0, i1, off, n_max = ref_pairs(name, shifted)
    p = our_pairs(name, shifted)
    n = len(SC.case(name).coords)
    assert p.index_0_offsets.dtype == torch.int32 and p.index_1.dtype == torch.int32
    assert torch.equal(p.index_0_offsets.long(), off) and p.n_max == n_max and p.m == i0.numel()
    # as sets per row: sort our rows the same way
    ours = p.index_0 * n + p.index_1.long()
    assert torch.equal(torch.sort(ours)[0], i0 * n + i1)
    # the order within a row: the small window ascending, then the large window ascending -- at most one descent per row
    descents = torch.zeros(n, dtype=torch.long, device="cuda").index_add_(
        0, p.index_0[1:], ((p.index_1[1:] <= p.index_1[:-1]) & (p.index_0[1:] == p.index_0[:-1])).long())
    assert int(descents.max()) <= 1
    # the transposed lists: a permutation of the pairs, grouped by key, ascending by pair within a key
    t_off, t_query, t_pair = p.by_key
    assert torch.equal(torch.sort(t_pair.long())[0], torch.arange(p.m, device="cuda"))
    key_of_slot = torch.repeat_interleave(torch.arange(n, device="cuda"), (t_off[1:] - t_off[:-1]).long())
    assert torch.equal(p.index_1.long()[t_pair.long()], key_of_slot)
    assert torch.equal(p.index_0[t_pair.long()], t_query.long())
    same_key = key_of_slot[1:] == key_of_slot[:-1]
    assert bool((t_pair[1:] > t_pair[:-1])[same_key].all())


def test_cases_take_the_paths_they_are_named_for():
    counts = {}
    for name in SC.NAMES:
        for shifted in (False, True):
            i0, i1, off, n_max = ref_pairs(name, shifted)
            _, ok = R.rel_index(_dev(SC.case(name).coords), i0, i1, SC.WINDOW, SC.QUANT)
            assert ok, "the reference's asserts on the relative index fail for %s" % name
            counts[name, shifted] = (off[1:] - off[:-1], n_max)
    assert int(counts["dense", False][0].min()) == 1           # a row of one pair, a query without large-window keys
    assert counts["dense", False][1] > 256                     # more than a workgroup's first pass
    assert int(((counts["dense", False][0] > 64) & (counts["dense", False][0] <= 256)).sum()) > 0   # more than a wave
    assert counts["long", False][1] > 1024                     # past the reference's cap


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", SC.NAMES)
def test_rel_index_equals_the_eager_statements(name, shifted):
    from ao_amd import stratified

    i0, i1, _, _ = ref_pairs(name, shifted)
    coords = _dev(SC.case(name).coords)
    want, ok = R.rel_index(coords, i0, i1, SC.WINDOW, SC.QUANT)
    assert ok
    got = stratified.rel_index(coords, i0, i1, SC.WINDOW, SC.QUANT, SC.ROWS)
    assert torch.equal(got.long(), want)


def test_rel_index_on_the_scale_of_the_reference_configs():
    """window 0.2 / quant 0.01 (tables of 80 rows), coordinates snapped to the quantisation grid: every relative position sits on
    an edge, where the reciprocal the device multiplies by decides the row"""
    from ao_amd import stratified

    rng = np.random.default_rng(5)
    coords = _dev((np.round(rng.uniform(0, 0.39, (300, 3)) / 0.01) * 0.01).astype(np.float32))
    i0 = torch.arange(300, device="cuda").repeat_interleave(300)
    i1 = torch.arange(300, device="cuda").repeat(300)
    want, ok = R.rel_index(coords, i0, i1, 0.2, 0.01)
    assert ok
    assert torch.equal(stratified.rel_index(coords, i0, i1, 0.2, 0.01).long(), want)


# ------------------------------------------------------------------------------------------ against float64 ----
def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def _peak(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def check(tag, res, f64, f32, keys):
    assert set(res) == keys and set(f64) == keys and set(f32) == keys
    bad = []
    for key in sorted(keys):
        assert torch.isfinite(res[key]).all(), key
        kinds = [("l2", _l2(res[key], f64[key]), _l2(f32[key], f64[key]))]
        if key in FWD_KEYS:
            kinds.append(("peak", _peak(res[key], f64[key]), _peak(f32[key], f64[key])))
        for kind, got, eager in kinds:
            allowed = M[key] * max(eager, FLOOR)
            print("st-ratio %-28s %-10s %-4s kernel %.3e  eager %.3e  ratio %.3f" % (tag, key, kind, got, eager, got / max(eager, FLOOR)))
            if not got <= allowed:
                bad.append((key, kind, got, allowed))
    assert not bad, bad


def _tensors(name, h, hd, dtype):
    t = {k: _dev(v) for k, v in SC.attention_inputs(SC.case(name), h, hd).items()}
    return {k: v.to(dtype) for k, v in t.items()}


LEAVES = ("q", "k", "v", "table_q", "table_k", "table_v")


def attention_reference(name, shifted, h, hd):
    """(float64, fp32) runs of st_ref.window_attention on the device, once per case"""
    key = ("attn", name, shifted, h, hd)
    if key not in _REF:
        for k in [k for k in _REF if k[0] == "attn"]:
            del _REF[k]
        i0, i1, _, _ = ref_pairs(name, shifted)
        coords = _dev(SC.case(name).coords)
        runs = []
        for dtype in (torch.float64, torch.float32):
            t = _tensors(name, h, hd, dtype)
            x = [t[k].requires_grad_(True) for k in LEAVES]
            out = R.window_attention(*x[:3], coords, i0, i1, *x[3:], SC.WINDOW, SC.QUANT)
            grads = torch.autograd.grad(out, x, t["g_out"])
            runs.append(dict(zip(["out"] + ["g_" + k for k in LEAVES], [out.detach()] + [g.detach() for g in grads])))
        _REF[key] = tuple(runs)
    return _REF[key]


def run_attention(name, shifted, h, hd):
    from ao_amd import stratified

    t = _tensors(name, h, hd, torch.float32)
    x = [t[k].requires_grad_(True) for k in LEAVES]
    out = stratified.window_attention(*x[:3], _dev(SC.case(name).coords), our_pairs(name, shifted), *x[3:], SC.WINDOW, SC.QUANT)
    assert out.dtype == torch.float32 and out.shape == (len(SC.case(name).coords), h * hd)
    grads = torch.autograd.grad(out, x, t["g_out"])
    return dict(zip(["out"] + ["g_" + k for k in LEAVES], [out.detach()] + [g.detach() for g in grads]))


ATTN_CASES = [("small", False), ("small", True), ("edges", False), ("edges", True), ("dense", False), ("dense", True), ("long", False)]


@pytest.mark.parametrize("path", ["fused", "staged", "torch"])
@pytest.mark.parametrize("name,shifted", ATTN_CASES)
def test_window_attention_against_float64(name, shifted, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_ST", path)
    f64, f32 = attention_reference(name, shifted, 2, 16)
    check("%s/%s/%s" % (name, "shift" if shifted else "plain", path), run_attention(name, shifted, 2, 16), f64, f32, ATTN_KEYS)


@pytest.mark.parametrize("name,shifted", [("small", True), ("dense", False)])
def test_window_attention_with_32_channels_takes_the_staged_operators(name, shifted, monkeypatch):
    monkeypatch.delenv("AO_AMD_ST", raising=False)
    f64, f32 = attention_reference(name, shifted, 2, 32)
    check("%s/%s/hd32" % (name, "shift" if shifted else "plain"), run_attention(name, shifted, 2, 32), f64, f32, ATTN_KEYS)


def _operator_runs(name, shifted, hd, which, ours):
    """one of the three operators: by st_ref in float64 and fp32, or (ours) by ao_amd.pointops2 with a FOREIGN CSR"""
    i0, i1, off, n_max = ref_pairs(name, shifted)
    coords = _dev(SC.case(name).coords)
    rel, _ = R.rel_index(coords, i0, i1, SC.WINDOW, SC.QUANT)
    n = len(SC.case(name).coords)
    runs = []
    for dtype in ([torch.float32] if ours else [torch.float64, torch.float32]):
        t = _tensors(name, 2, hd, dtype)
        gen = torch.Generator(device="cuda").manual_seed(3)
        attn = torch.softmax(torch.randn((i0.numel(), 2), device="cuda", generator=gen, dtype=torch.float64), 0).mul(50.0).to(dtype)
        g_pairs = torch.randn((i0.numel(), 2), device="cuda", generator=gen, dtype=torch.float64).to(dtype)
        if ours:
            from ao_amd.pointops2 import pointops as P2

            o32, i32, r32 = off.int(), i1.int(), rel.int()
        if which == "step1":
            x = [t[k].requires_grad_(True) for k in ("q", "k")]
            out = P2.attention_step1_v2(*x, i32, o32, n_max) if ours else R.attention_step1(*x, i0, i1)
            names, g = ["out", "g_q", "g_k"], g_pairs
        elif which == "dot":
            x = [t[k].requires_grad_(True) for k in ("q", "k", "table_q", "table_k")]
            out = P2.dot_prod_with_idx_v3(x[0], o32, n_max, x[1], i32, x[2], x[3], r32) if ours else \
                R.dot_prod_with_idx(x[0], x[1], i0, i1, x[2], x[3], rel)
            names, g = ["out", "g_q", "g_k", "g_table_q", "g_table_k"], g_pairs
        else:
            x = [attn.requires_grad_(True)] + [t[k].requires_grad_(True) for k in ("v", "table_v")]
            out = P2.attention_step2_with_rel_pos_value_v2(x[0], x[1], o32, n_max, i32, x[2], r32) if ours else \
                R.attention_step2(x[0], x[1], i0, i1, x[2], rel)
            names, g = ["out", "g_attn", "g_v", "g_table_v"], t["g_out"].view(n, 2, hd)
        grads = torch.autograd.grad(out, x, g)
        runs.append(dict(zip(names, [out.detach()] + [gr.detach() for gr in grads])))
    return runs


@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("which", ["step1", "dot", "step2"])
@pytest.mark.parametrize("name,shifted", [("small", False), ("edges", True), ("dense", False), ("long", False)])
def test_pointops2_operator_against_float64(name, shifted, which, hd):
    f64, f32 = _operator_runs(name, shifted, hd, which, False)
    (res,) = _operator_runs(name, shifted, hd, which, True)
    check("%s/%s/%s/hd%d" % (name, "shift" if shifted else "plain", which, hd), res, f64, f32, set(f64))


@pytest.mark.parametrize("name", ["edges", "dense"])
def test_scatter_softmax_against_float64(name):
    from ao_amd import stratified

    i0, _, off, _ = ref_pairs(name, False)
    n = len(SC.case(name).coords)
    gen = torch.Generator(device="cuda").manual_seed(4)
    src64 = torch.randn((i0.numel(), 2), device="cuda", generator=gen, dtype=torch.float64) * 3
    g64 = torch.randn((i0.numel(), 2), device="cuda", generator=gen, dtype=torch.float64)
    runs = []
    for dtype, ours in ((torch.float64, False), (torch.float32, False), (torch.float32, True)):
        x = src64.to(dtype).requires_grad_(True)
        out = stratified.scatter_softmax_csr(x, off.int()) if ours else R.scatter_softmax(x, i0, n)
        runs.append({"out": out.detach(), "g_attn": torch.autograd.grad(out, x, g64.to(dtype))[0].detach()})
    check("%s/softmax" % name, runs[2], runs[0], runs[1], {"out", "g_attn"})


# ------------------------------------------------------------------------------- repeatability and memory ----
def test_fused_runs_repeat_bit_for_bit(monkeypatch):
    monkeypatch.setenv("AO_AMD_ST", "fused")
    a, b = run_attention("dense", False, 2, 16), run_attention("dense", False, 2, 16)
    for key in ("out", "g_q", "g_k", "g_v"):
        assert torch.equal(a[key], b[key]), key


def test_fused_allocates_nothing_of_the_size_of_the_pairs(monkeypatch):
    """`long` has 1.08 million pairs: one (M, h) fp32 array is 8.7 MB, the (M, 3) index 13 MB, while q, k, v, out and their
    gradients are 145 kB each.  Forward and backward of the fused node may allocate an eighth of one (M, h) array."""
    from ao_amd import stratified

    monkeypatch.setenv("AO_AMD_ST", "fused")
    pairs = our_pairs("long", False)
    t = _tensors("long", 2, 16, torch.float32)
    x = [t[k].requires_grad_(True) for k in LEAVES]
    coords = _dev(SC.case("long").coords)
    one = pairs.m * 2 * 4
    assert one > 8e6

    def step():
        out = stratified.window_attention(*x[:3], coords, pairs, *x[3:], SC.WINDOW, SC.QUANT)
        return torch.autograd.grad(out, x, t["g_out"])

    step()   # the library is loaded, nothing is cached after this
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    grads = step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print("st-memory fused: peak %d bytes above the inputs, one (M, h) array is %d" % (extra, one))
    assert extra < one // 8, (extra, one)
    del grads


def test_unprovided_pointops2_names_raise():
    from ao_amd.pointops2 import pointops as P2

    for name in ("attention_step1", "attention_step2", "attention_step2_v2", "dot_prod_with_idx", "dot_prod_with_idx_v2",
                 "attention_step2_with_rel_pos_value"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(P2, name)()
