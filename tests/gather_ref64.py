"""float64 statements of the 18 contracts of ao_amd/csrc/gather_ops.hip (14) and ao_amd/csrc/pool.hip (4), written from
include/ptv2_hip.h: grouping, interpolation and its weights, subtraction, aggregation, the attention relation / fusion steps,
segment_minmax, pool_max forward / backward, segment_sum.

Every statement takes the dict of a case's fp32 / int32 numpy inputs (tests/gather_cases.py), a dtype and an optional mutation:

    fn(t, dt=np.float64, mut=None) -> {output name: Sum | ndarray}

* dt = float64 is the reference.  dt = float32 forms every TERM with fp32 roundings (one per operation, as the kernels do
  without contraction); `emulate` then adds the terms of every element one after the other in fp32 in a chosen order.  That
  pair is the fp32 model tests/test_gather_ref64_host.py holds to the bound, and the carrier of the deliberately wrong
  variants (`mut`) that prove the bound and the exact tier notice them.
* An output that is a sum is a `Sum`: the element -> terms relation itself, from which value (float64), T (number of terms) and
  A (sum of |term|) follow.  `factors` is the number of input operands multiplied in a term (the fractional bits of a term on
  the exact tier are factors x bits), `ops` the number of fp32 roundings it takes to form one term.
* Outputs that are copies or selections are plain arrays.

Bounds (DESIGN.md 3.4 "Parity against float64: gather and pooling kernels"):

    rounding tier   |kernel - value| <= (T + 2) 2^-24 A            per element; T == 1 and ops <= 1: correctly rounded
    exact tier      kernel == float32(value) bit for bit           (every partial sum representable: A 2^f an integer < 2^24)
    weights         |kernel - value| <= (k + 3) 2^-24 |value|      interpolation_weights
"""
import numpy as np

F64, F32 = np.float64, np.float32
U = 2.0 ** -24


class Sum:
    """element d (flat index into `shape`) is the sum of term[i] over the i with dest[i] == d"""

    def __init__(self, shape, dest, term, factors, ops):
        self.shape = tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.dest = np.ascontiguousarray(dest, dtype=np.int64).ravel()
        self.term = np.ascontiguousarray(term).ravel()
        self.factors, self.ops = factors, ops
        assert self.dest.shape == self.term.shape
        assert self.dest.size == 0 or (0 <= self.dest.min() and self.dest.max() < self.size)

    def _bin(self, w):
        return np.bincount(self.dest, weights=w, minlength=self.size).astype(F64).reshape(self.shape)

    @property
    def value(self):
        return self._bin(self.term.astype(F64))

    @property
    def T(self):
        return self._bin(None)

    @property
    def A(self):
        return self._bin(np.abs(self.term.astype(F64)))

    def bound(self):
        return (self.T + 2.0) * U * self.A


def emulate(s, order, rng):
    """the fp32 sum of every element of Sum `s` (terms already fp32), one term after the other, in `order`: 'random',
    'ascending' or 'descending' magnitude"""
    term, dest = s.term.astype(F32), s.dest
    acc = np.zeros(s.size, F32)
    if term.size == 0:
        return acc.reshape(s.shape)
    second = {"random": rng.permutation(term.size), "ascending": np.abs(term), "descending": -np.abs(term)}[order]
    o = np.lexsort((second, dest))
    d, v = dest[o], term[o]
    start = np.r_[0, np.flatnonzero(d[1:] != d[:-1]) + 1]
    pos = np.arange(d.size) - np.repeat(start, np.diff(np.r_[start, d.size]))
    by_pos = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[by_pos], np.arange(int(pos.max()) + 2))
    for p in range(cuts.size - 1):   # the p-th term of every element at once: every element at most once per pass
        sel = by_pos[cuts[p]:cuts[p + 1]]
        acc[d[sel]] = acc[d[sel]] + v[sel]
    return acc.reshape(s.shape)


def realise(out, order="random", rng=None):
    """a statement's dict with every Sum replaced by an array: float64 values, or the fp32 emulation where the terms are fp32"""
    rng = rng or np.random.default_rng(0)
    res = {}
    for key, o in out.items():
        if isinstance(o, Sum):
            res[key] = emulate(o, order, rng) if o.term.dtype == F32 else o.value
        else:
            res[key] = o
    return res


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == F32:
        return bool(np.array_equal(a.view(np.int32), b.view(np.int32)))
    return bool(np.array_equal(a, b))


def to_f32(value):
    """the correctly rounded fp32 of a float64 reference value (integer outputs pass through)"""
    return value.astype(F32) if value.dtype == F64 else value


def compare(got, ref, tier):
    """(ok, worst err / bound, message) of one output: `got` the fp32 / int32 array under test, `ref` the float64 statement's
    Sum or array.  Exact tier and selections: bit equality with the rounded reference.  Rounding tier, sums: the bound per
    element, and where one term of at most one rounding makes the element, correct rounding."""
    got = np.ascontiguousarray(got)
    if not isinstance(ref, Sum):
        want = to_f32(ref)
        if got.shape != want.shape:
            return False, float("inf"), "shape %s, expected %s" % (got.shape, want.shape)
        ok = bits_equal(got, want)
        return ok, 0.0 if ok else float("inf"), "" if ok else _first_difference(got, want)
    value = ref.value
    if got.shape != value.shape:
        return False, float("inf"), "shape %s, expected %s" % (got.shape, value.shape)
    if tier == "exact":
        want = value.astype(F32)
        ok = bits_equal(got, want)
        return ok, 0.0 if ok else float("inf"), "" if ok else _first_difference(got, want)
    if not np.isfinite(got).all():
        return False, float("inf"), "not finite (an unwritten element shows as NaN)"
    err, bound, terms = np.abs(got.astype(F64) - value), ref.bound(), ref.T
    bad = err > bound
    if ref.ops <= 1:
        bad |= (terms == 1) & (got != value.astype(F32))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        return False, ratio, (
            "%d elements out of bound, first flat index %d: got %r, float64 %r, T %d, A %r, bound %r" % (
                int(bad.sum()), i, float(got.ravel()[i]), float(value.ravel()[i]), int(terms.ravel()[i]),
                float(ref.A.ravel()[i]), float(bound.ravel()[i])))
    return True, ratio, ""


def _first_difference(got, want):
    g, w = got.ravel(), want.ravel()
    same = (g.view(np.int32) == w.view(np.int32)) if g.dtype == F32 else (g == w)
    i = int(np.flatnonzero(~same)[0])
    return "%d of %d elements differ in their bits, first flat index %d: got %r, expected %r" % (
        int((~same).sum()), g.size, i, g[i].item(), w[i].item())


# ------------------------------------------------------------------------------------------------------------------- helpers
def _grid(*dims):
    return np.ix_(*[np.arange(d, dtype=np.int64) for d in dims])


def _rows(idx, mut):
    """the `idx row shifted by one` mutation: row r reads the index row of r - 1"""
    return np.roll(idx, 1, axis=0) if mut == "shift" else idx


def _full(a, shape):
    return np.broadcast_to(a, shape)


def inverse_table(idx, m):
    """CSR inverse of idx (n, k) with entries in [0, m) (include/ptv2_hip.h, inverse_table): the slots r = n k + i with
    idx[r] == j are inv_rows[inv_ptr[j] : inv_ptr[j + 1]], ascending"""
    flat = idx.ravel().astype(np.int64)
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < m)
    inv_rows = np.argsort(flat, kind="stable").astype(np.int32)
    inv_ptr = np.r_[0, np.cumsum(np.bincount(flat, minlength=m))].astype(np.int32)
    return inv_ptr, inv_rows


# ------------------------------------------------------------------------------------------------------------------ grouping
def grouping_forward(t, dt=F64, mut=None):
    """output[m,s,:] = input[idx[m,s],:], zeros where idx < 0"""
    x, idx = t["input"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    out = np.where((idx >= 0)[..., None], x[np.maximum(idx, 0)], dt(0))
    if mut == "drop_last":
        out[:, -1] = 0
    return dict(output=out)


def grouping_backward(t, dt=F64, mut=None):
    """grad_input[idx[m,s],:] += grad_output[m,s,:]"""
    go, idx = t["grad_output"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    m, ns, c = go.shape
    _, S, C = _grid(m, ns, c)
    keep = _full(idx[..., None] >= 0, go.shape)
    if mut == "drop_last":
        keep = keep & (S < ns - 1)
    dest = _full(idx[..., None] * c + C, go.shape)
    return dict(grad_input=Sum((t["n"], c), dest[keep], go[keep], 1, 0))


# ------------------------------------------------------------------------------------------------------------- interpolation
def interpolation_weights(t, dt=F64, mut=None):
    """weight[i,s] = r_s / sum_t r_t, r_s = 1 / (sqrt(dist2[i,s]) + 1e-8f), the sum in slot order; idx < 0 -> idx + n"""
    d2, idx = t["dist2"].astype(dt), t["idx"]
    r = dt(1) / (np.sqrt(d2) + dt(F32(1e-8)))
    norm = np.zeros(d2.shape[0], dt)
    for s in range(d2.shape[1]):
        norm = norm + r[:, s]
    if mut == "norm_k":
        norm = np.full_like(norm, d2.shape[1])
    return dict(weight=r / norm[:, None], idx=np.where(idx < 0, idx + t["n"], idx).astype(np.int32))


def interpolation_forward(t, dt=F64, mut=None):
    """output[n,:] += sum_i input[idx[n,i],:] * weight[n,i]"""
    x, w, idx = t["input"].astype(dt), t["weight"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    n, k = idx.shape
    c = x.shape[1]
    N, I, C = _grid(n, k, c)
    term = x[idx] * w[..., None]
    keep = _full(I < (k - 1 if mut == "drop_last" else k), term.shape)
    dest = _full(N * c + C, term.shape)
    return dict(output=Sum((n, c), dest[keep], term[keep], 2, 1))


def interpolation_backward(t, dt=F64, mut=None):
    """grad_input[idx[n,i],:] += grad_output[n,:] * weight[n,i]       grad_input (m, c)"""
    go, w, idx = t["grad_output"].astype(dt), t["weight"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    n, k = idx.shape
    c = go.shape[1]
    N, I, C = _grid(n, k, c)
    rows = _full(N, (n, k, 1))[..., 0]
    if mut == "r_mod_k":   # slot r = n k + i read as row r % k of grad_output
        rows = _full(I % max(n, 1), (n, k, 1))[..., 0]
    term = go[rows] * w[..., None]
    keep = _full(I < (k - 1 if mut == "drop_last" else k), term.shape)
    dest = _full(idx[..., None] * c + C, term.shape)
    return dict(grad_input=Sum((t["m"], c), dest[keep], term[keep], 2, 1))


interpolation_backward_gather = interpolation_backward   # the same gradient, gathered through the inverse table


# --------------------------------------------------------------------------------------------------------------- subtraction
def subtraction_forward(t, dt=F64, mut=None):
    """output[n,s,:] = input1[n,:] - input2[idx[n,s],:]"""
    a, b, idx = t["input1"].astype(dt), t["input2"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    return dict(output=a[:, None, :] - b[idx])


def subtraction_backward(t, dt=F64, mut=None):
    """grad_input1[n,:] += g, grad_input2[idx[n,s],:] -= g, g = grad_output[n,s,:]"""
    go, idx = t["grad_output"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    n, ns, c = go.shape
    N, S, C = _grid(n, ns, c)
    keep = _full(S < (ns - 1 if mut == "drop_last" else ns), go.shape)
    d1, d2 = _full(N * c + C, go.shape), _full(idx[..., None] * c + C, go.shape)
    return dict(grad_input1=Sum((n, c), d1[keep], go[keep], 1, 0), grad_input2=Sum((n, c), d2[keep], -go[keep], 1, 0))


# --------------------------------------------------------------------------------------------------------------- aggregation
def _weight_channel(c, w_c, mut):
    ci = np.arange(c, dtype=np.int64)
    if mut == "wc_div":   # `ci / (c / w_c)` written for `ci % w_c`
        return np.minimum(ci // max(c // w_c, 1), w_c - 1)
    return ci % w_c


def aggregation_forward(t, dt=F64, mut=None):
    """output[n,c] += sum_s (input[idx[n,s],c] + position[n,s,c]) * weight[n,s,c % w_c]"""
    x, p, w, idx = t["input"].astype(dt), t["position"].astype(dt), t["weight"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    n, ns, c = p.shape
    wi = _weight_channel(c, w.shape[2], mut)
    N, S, C = _grid(n, ns, c)
    term = (x[idx] + p) * w[:, :, wi]
    keep = _full(S < (ns - 1 if mut == "drop_last" else ns), term.shape)
    dest = _full(N * c + C, term.shape)
    return dict(output=Sum((n, c), dest[keep], term[keep], 2, 2))


def aggregation_backward(t, dt=F64, mut=None):
    """grad_input[idx[n,s],c] += go[n,c] w[n,s,c % w_c]; grad_position[n,s,c] = go[n,c] w[n,s,c % w_c];
    grad_weight[n,s,wi] += sum over the c with c % w_c == wi of go[n,c] (input[idx[n,s],c] + position[n,s,c])"""
    x, p, w, idx = t["input"].astype(dt), t["position"].astype(dt), t["weight"].astype(dt), _rows(t["idx"], mut).astype(np.int64)
    go = t["grad_output"].astype(dt)
    n, ns, c = p.shape
    w_c = w.shape[2]
    wi = _weight_channel(c, w_c, mut)
    N, S, C = _grid(n, ns, c)
    gpos = go[:, None, :] * w[:, :, wi]
    gw = go[:, None, :] * (x[idx] + p)
    keep = _full(S < (ns - 1 if mut == "drop_last" else ns), gpos.shape)
    d_in = _full(idx[..., None] * c + C, gpos.shape)
    d_w = _full((N * ns + S) * w_c + wi[None, None, :], gpos.shape)
    if mut == "drop_last":
        gpos = np.where(keep, gpos, dt(0))
    return dict(grad_input=Sum((x.shape[0], c), d_in[keep], gpos[keep], 2, 1), grad_position=gpos,
                grad_weight=Sum((n, ns, w_c), d_w[keep], gw[keep], 2, 2))


# ----------------------------------------------------------------------------------------------------------------- attention
def _edges(t, mut):
    tgt, ref = t["index_target"].astype(np.int64), t["index_refer"].astype(np.int64)
    if mut == "shift":
        tgt, ref = np.roll(tgt, 1), np.roll(ref, 2)
    return tgt, ref


def attention_relation_step_forward(t, dt=F64, mut=None):
    """output[r,g] += sum_c query[tgt[r],g,c] * key[ref[r],g,c] * weight[c]"""
    q, k, w = t["query"].astype(dt), t["key"].astype(dt), t["weight"].astype(dt)
    tgt, ref = _edges(t, mut)
    m, (_, g, c) = tgt.shape[0], q.shape
    R, G, C = _grid(m, g, c)
    term = q[tgt] * k[ref] * w
    keep = _full(C < (c - 1 if mut == "drop_last" else c), term.shape)
    dest = _full(R * g + G, term.shape)
    return dict(output=Sum((m, g), dest[keep], term[keep], 3, 2))


def attention_relation_step_backward(t, dt=F64, mut=None):
    """grad_query[tgt[r],g,c] += go[r,g] key[ref[r],g,c] weight[c]; grad_key[ref[r],g,c] += go[r,g] query[tgt[r],g,c] weight[c];
    grad_weight[c] += go[r,g] key[ref[r],g,c] query[tgt[r],g,c]"""
    q, k, w, go = t["query"].astype(dt), t["key"].astype(dt), t["weight"].astype(dt), t["grad_output"].astype(dt)
    tgt, ref = _edges(t, mut)
    m, (n, g, c) = tgt.shape[0], q.shape
    R, G, C = _grid(m, g, c)
    gr = go[:, :, None]
    shape = (m, g, c)
    keep = _full(R < (m - 1 if mut == "drop_last" else m), shape)
    dq = _full((tgt[:, None, None] * g + G) * c + C, shape)
    dk = _full((ref[:, None, None] * g + G) * c + C, shape)
    dw = _full(C, shape)
    return dict(grad_query=Sum((n, g, c), dq[keep], (gr * k[ref] * w)[keep], 3, 2),
                grad_key=Sum((n, g, c), dk[keep], (gr * q[tgt] * w)[keep], 3, 2),
                grad_weight=Sum((c,), dw[keep], (gr * k[ref] * q[tgt])[keep], 3, 2))


def attention_fusion_step_forward(t, dt=F64, mut=None):
    """output[tgt[r],g,c] += weight[r,g] * value[ref[r],g,c]"""
    w, v = t["weight"].astype(dt), t["value"].astype(dt)
    tgt, ref = _edges(t, mut)
    m, (n, g, c) = tgt.shape[0], v.shape
    R, G, C = _grid(m, g, c)
    term = w[:, :, None] * v[ref]
    keep = _full(R < (m - 1 if mut == "drop_last" else m), term.shape)
    dest = _full((tgt[:, None, None] * g + G) * c + C, term.shape)
    return dict(output=Sum((n, g, c), dest[keep], term[keep], 2, 1))


def attention_fusion_step_backward(t, dt=F64, mut=None):
    """grad_weight[r,g] += sum_c go[tgt[r],g,c] value[ref[r],g,c]; grad_value[ref[r],g,c] += go[tgt[r],g,c] weight[r,g]"""
    w, v, go = t["weight"].astype(dt), t["value"].astype(dt), t["grad_output"].astype(dt)
    tgt, ref = _edges(t, mut)
    m, (n, g, c) = tgt.shape[0], v.shape
    R, G, C = _grid(m, g, c)
    shape = (m, g, c)
    keep = _full(C < (c - 1 if mut == "drop_last" else c), shape)
    dw = _full(R * g + G, shape)
    dv = _full((ref[:, None, None] * g + G) * c + C, shape)
    return dict(grad_weight=Sum((m, g), dw[keep], (go[tgt] * v[ref])[keep], 2, 1),
                grad_value=Sum((n, g, c), dv[keep], (go[tgt] * w[:, :, None])[keep], 2, 1))


# ------------------------------------------------------------------------------------------------------------------- pooling
def _members(t, mut):
    """(cluster of every CSR slot, position of the slot inside its cluster, row of the slot), last member dropped on request"""
    order, ptr = t["order"].astype(np.int64), t["idx_ptr"].astype(np.int64)
    length = np.diff(ptr)
    assert (length >= 1).all(), "a cluster has at least one member (include/ptv2_hip.h)"
    cluster = np.repeat(np.arange(length.size), length)
    pos = np.arange(order.size) - ptr[cluster]
    keep = np.ones(order.size, bool)
    if mut == "drop_last":
        keep = (pos < length[cluster] - 1) | (length[cluster] == 1)
    return cluster[keep], pos[keep], order[keep]


def pool_max_forward(t, dt=F64, mut=None):
    """out[j,:] = max over the members of cluster j in `order`, arg = the winning row: a sequential `>` scan, so the first
    member wins ties (and a -0.0 met first is kept against a later +0.0)"""
    feat = t["feat"].astype(dt)
    cluster, pos, row = _members(t, mut)
    n_out, c = t["idx_ptr"].size - 1, feat.shape[1]
    out, arg = np.zeros((n_out, c), dt), np.zeros((n_out, c), np.int32)
    for p in range(int(pos.max()) + 1 if pos.size else 0):
        sel = pos == p
        j, v = cluster[sel], feat[row[sel]]
        if p == 0:
            out[j], arg[j] = v, row[sel][:, None]
            continue
        better = (v >= out[j]) if mut == "tie_last" else (v > out[j])
        out[j] = np.where(better, v, out[j])
        arg[j] = np.where(better, row[sel][:, None], arg[j])
    return dict(out=out, arg=arg)


def pool_max_backward(t, dt=F64, mut=None):
    """grad_feat[arg[j,c], c] = grad_out[j,c], zeros elsewhere (every (j, c) owns its destination)"""
    go, arg = t["grad_out"].astype(dt), _rows(t["arg"], mut).astype(np.int64)
    gf = np.zeros((t["n_in"], go.shape[1]), dt)
    gf[arg, _full(np.arange(go.shape[1]), arg.shape)] = go
    return dict(grad_feat=gf)


def segment_sum(t, dt=F64, mut=None):
    """grad_coarse[j,:] = sum over the members of cluster j of grad_fine"""
    gf = t["grad_fine"].astype(dt)
    cluster, _, row = _members(t, mut)
    c = gf.shape[1]
    term = gf[row]
    dest = cluster[:, None] * c + np.arange(c)[None, :]
    return dict(grad_coarse=Sum((t["idx_ptr"].size - 1, c), dest, term, 1, 0))


def segment_minmax(t, dt=F64, mut=None):
    """lo / hi (b, 3): per-cloud coordinate minimum and maximum"""
    xyz, off = t["xyz"].astype(dt), t["offset"].astype(np.int64)
    lo, hi = np.zeros((off.size, 3), dt), np.zeros((off.size, 3), dt)
    for s, (a, b) in enumerate(zip(np.r_[0, off[:-1]], off)):
        seg = xyz[a:b - 1] if mut == "drop_last" and b - a > 1 else xyz[a:b]
        lo[s], hi[s] = seg.min(0), seg.max(0)
    return dict(lo=lo, hi=hi)


CONTRACTS = dict(
    grouping_forward_hip_launcher=grouping_forward,
    grouping_backward_hip_launcher=grouping_backward,
    interpolation_weights_hip_launcher=interpolation_weights,
    interpolation_forward_hip_launcher=interpolation_forward,
    interpolation_backward_hip_launcher=interpolation_backward,
    interpolation_backward_gather_hip_launcher=interpolation_backward_gather,
    subtraction_forward_hip_launcher=subtraction_forward,
    subtraction_backward_hip_launcher=subtraction_backward,
    aggregation_forward_hip_launcher=aggregation_forward,
    aggregation_backward_hip_launcher=aggregation_backward,
    attention_relation_step_forward_hip_launcher=attention_relation_step_forward,
    attention_relation_step_backward_hip_launcher=attention_relation_step_backward,
    attention_fusion_step_forward_hip_launcher=attention_fusion_step_forward,
    attention_fusion_step_backward_hip_launcher=attention_fusion_step_backward,
    segment_minmax_hip_launcher=segment_minmax,
    pool_max_forward_hip_launcher=pool_max_forward,
    pool_max_backward_hip_launcher=pool_max_backward,
    segment_sum_hip_launcher=segment_sum,
)

# the outputs compared for every launcher (asserted against what a run returns)
KEYS = dict(
    grouping_forward_hip_launcher=("output",),
    grouping_backward_hip_launcher=("grad_input",),
    interpolation_weights_hip_launcher=("weight", "idx"),
    interpolation_forward_hip_launcher=("output",),
    interpolation_backward_hip_launcher=("grad_input",),
    interpolation_backward_gather_hip_launcher=("grad_input",),
    subtraction_forward_hip_launcher=("output",),
    subtraction_backward_hip_launcher=("grad_input1", "grad_input2"),
    aggregation_forward_hip_launcher=("output",),
    aggregation_backward_hip_launcher=("grad_input", "grad_position", "grad_weight"),
    attention_relation_step_forward_hip_launcher=("output",),
    attention_relation_step_backward_hip_launcher=("grad_query", "grad_key", "grad_weight"),
    attention_fusion_step_forward_hip_launcher=("output",),
    attention_fusion_step_backward_hip_launcher=("grad_weight", "grad_value"),
    segment_minmax_hip_launcher=("lo", "hi"),
    pool_max_forward_hip_launcher=("out", "arg"),
    pool_max_backward_hip_launcher=("grad_feat",),
    segment_sum_hip_launcher=("grad_coarse",),
)

# which deliberately wrong variants a contract has (tests/test_gather_ref64_host.py runs each on every case it changes)
MUTANTS = dict(
    grouping_forward_hip_launcher=("drop_last", "shift"),
    grouping_backward_hip_launcher=("drop_last", "shift"),
    interpolation_weights_hip_launcher=("norm_k",),
    interpolation_forward_hip_launcher=("drop_last", "shift"),
    interpolation_backward_hip_launcher=("drop_last", "shift"),
    interpolation_backward_gather_hip_launcher=("drop_last", "r_mod_k"),
    subtraction_forward_hip_launcher=("shift",),
    subtraction_backward_hip_launcher=("drop_last", "shift"),
    aggregation_forward_hip_launcher=("drop_last", "shift", "wc_div"),
    aggregation_backward_hip_launcher=("drop_last", "shift", "wc_div"),
    attention_relation_step_forward_hip_launcher=("drop_last", "shift"),
    attention_relation_step_backward_hip_launcher=("drop_last", "shift"),
    attention_fusion_step_forward_hip_launcher=("drop_last", "shift"),
    attention_fusion_step_backward_hip_launcher=("drop_last", "shift"),
    segment_minmax_hip_launcher=("drop_last",),
    pool_max_forward_hip_launcher=("tie_last", "drop_last"),
    pool_max_backward_hip_launcher=("shift",),
    segment_sum_hip_launcher=("drop_last",),
)


def weights_bound(k):
    """relative, per weight: sqrt, add and divide at half a unit each, k - 1 additions in the norm, the final divide"""
    return (k + 3) * U


def compare_weights(got, value, k):
    """(ok, worst err / bound, message) for interpolation_weights' `weight`"""
    got = np.ascontiguousarray(got)
    if got.shape != value.shape:
        return False, float("inf"), "shape %s, expected %s" % (got.shape, value.shape)
    if got.size == 0:
        return True, 0.0, ""
    if not np.isfinite(got).all():
        return False, float("inf"), "not finite (an unwritten element shows as NaN)"
    err, bound = np.abs(got.astype(F64) - value), weights_bound(k) * np.abs(value)
    ratio = float((err / bound).max())
    if (err > bound).any():
        i = int(np.flatnonzero((err > bound).ravel())[0])
        return False, ratio, "%d weights out of bound, first flat index %d: got %r, float64 %r" % (
            int((err > bound).sum()), i, float(got.ravel()[i]), float(value.ravel()[i]))
    return True, ratio, ""
