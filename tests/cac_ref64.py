"""float64 statements of the contracts of ao_amd/csrc/cac.hip (six launchers) and ao_amd/csrc/loss.hip (two), written from the
contract text of include/ptv2_hip.h: weighted sums (soft prototypes / class means) forward and backward, cosine logits forward and
backward, the distillation loss forward and backward, softmax cross-entropy forward and backward.

Every statement takes the dict of a case's fp32 / int numpy inputs (tests/cac_cases.py), a dtype and an optional mutation:

    fn(t, dt=np.float64, mut=None) -> {output name: V | ndarray}

* dt = float64 is the reference.  Every quantity is a `V`: the value, its magnitude `a` (the same expression with every added
  term replaced by its absolute value) and `e`, the bound on |fp32 evaluation - value|.  `e` is not fitted: it follows from the
  operations, by the rules below, and an inner quantity's `e` is carried into the outer one by the derivative of the outer
  expression (the softmax weight into the prototype sum, `lse` into the loss row, the forward's z / out / coef / lse into the
  backward that reads them).  Unrolled, e <= (T + S) 2^-24 a plus the carried part (DESIGN.md 3.8c gives T and S per output).
* dt = float32 is the fp32 emulation (`E32`): numpy fp32, one rounding per operation, every sum added one term after the
  other; the row sums in the order `EMU["order"]`: "chunks" (256-row chunks, then the slabs of a set in order: the kernels'),
  "rows" or "random".  It carries the deliberately wrong variants (`mut`) of tests/test_cac_ref64_host.py.
* Outputs that are exact (counts, the number of bad labels) are plain arrays and compare bit for bit.

RULES (u = 2^-24; inputs are fp32 numbers: e = 0)

    a + b, a - b     e = e_a + e_b + u (|v| + e_a + e_b)                      one rounding of the result
    a * b            e = |a| e_b + |b| e_a + e_a e_b, then one rounding
    sum of T terms   e = sum e_i + g(T - 1) sum (|v_i| + e_i),  g(m) = m u / (1 - m u)     any order, any tree
    a / b            e = (e_a + |a / b| e_b) / (|b| - e_b), then ELEM roundings
    exp, log, sqrt   the exact propagation of e through the function, then ELEM roundings; exp adds 2^-126 absolute (a
                     subnormal result may be flushed)

ELEM = 8: four units in the last place (a unit is at most 2^-23 relative) for each expf, logf, sqrtf and division.  The
device library documents 1 ulp for expf and logf and correct rounding for sqrtf and the division (ROCm OCML, "Precision of
math functions"); four is generous against that and still three orders of magnitude below what an indexing mistake produces.
The constants 1e-12 (norm clamp), 1e-4 (distillation) and the eps arguments are the fp32 numbers the kernels receive."""
import numpy as np

F64, F32 = np.float64, np.float32
U = 2.0 ** -24
ELEM = 8.0
TINY = 2.0 ** -126
CHUNK = 256
# constants and scalar arguments are the fp32 numbers the kernels receive; the host test sets F64 here to compare the statements
# with the eager formulations run in float64, which take 1e-12, 1e-4 and eps as doubles
ROUND = F32


def _c(x):
    return F64(ROUND(x))


# how the fp32 emulation orders the terms of a row sum: "chunks", "rows" or "random" (with `rng`)
EMU = dict(order="rows", rng=None)


def gamma(m):
    m = np.maximum(np.asarray(m, F64), 0.0)
    return m * U / (1.0 - m * U)


class V:
    """float64 value `v`, magnitude `a`, bound `e` on the error of an fp32 evaluation"""

    def __init__(self, v, a=None, e=None):
        self.v = np.asarray(v, F64)
        self.a = np.abs(self.v) if a is None else np.asarray(a, F64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, F64)

    shape = property(lambda s: s.v.shape)

    @staticmethod
    def _rounded(v, a, e, units=1.0):
        return V(v, a, e + units * U * (np.abs(v) + e))

    def lift(self, o):
        return o if isinstance(o, V) else V(np.asarray(o, F64))

    def __add__(self, o):
        o = self.lift(o)
        return V._rounded(self.v + o.v, self.a + o.a, self.e + o.e)

    def __sub__(self, o):
        o = self.lift(o)
        return V._rounded(self.v - o.v, self.a + o.a, self.e + o.e)

    def __neg__(self):
        return V(-self.v, self.a, self.e)

    def __mul__(self, o):
        o = self.lift(o)
        return V._rounded(self.v * o.v, self.a * o.a, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = self.lift(o)
        with np.errstate(all="ignore"):
            q, ad = self.v / o.v, np.abs(o.v)
            return V._rounded(q, self.a / ad, (self.e + np.abs(q) * o.e) / (ad - o.e), ELEM)

    def sum(self, axis, keepdims=False):
        mag = (np.abs(self.v) + self.e).sum(axis, keepdims=keepdims)
        return V(self.v.sum(axis, keepdims=keepdims), self.a.sum(axis, keepdims=keepdims),
                 self.e.sum(axis, keepdims=keepdims) + gamma(self.v.shape[axis] - 1) * mag)

    def __getitem__(self, i):
        return V(self.v[i], self.a[i], self.e[i])

    def t(self):
        return V(np.swapaxes(self.v, -1, -2), np.swapaxes(self.a, -1, -2), np.swapaxes(self.e, -1, -2))

    def reshape(self, *s):
        return V(self.v.reshape(*s), self.a.reshape(*s), self.e.reshape(*s))


class E32:
    """the fp32 emulation: one numpy fp32 operation per operation of the statement"""

    def __init__(self, v):
        self.v = np.asarray(v, F32)

    shape = property(lambda s: s.v.shape)

    def lift(self, o):
        return o if isinstance(o, E32) else E32(np.asarray(o, F32))

    def __add__(self, o):
        return E32(self.v + self.lift(o).v)

    def __sub__(self, o):
        return E32(self.v - self.lift(o).v)

    def __neg__(self):
        return E32(-self.v)

    def __mul__(self, o):
        return E32(self.v * self.lift(o).v)

    def __truediv__(self, o):
        with np.errstate(all="ignore"):
            return E32(self.v / self.lift(o).v)

    def sum(self, axis, keepdims=False):
        acc = np.zeros(np.delete(self.v.shape, axis if axis >= 0 else self.v.ndim + axis), F32)
        for i in range(self.v.shape[axis]):
            acc = acc + np.take(self.v, i, axis)
        return E32(np.expand_dims(acc, axis) if keepdims else acc)

    def __getitem__(self, i):
        return E32(self.v[i])

    def t(self):
        return E32(np.swapaxes(self.v, -1, -2))

    def reshape(self, *s):
        return E32(self.v.reshape(*s))


def inp(x, dt):
    return V(x) if dt is F64 else E32(x)


def exp(x):
    if isinstance(x, E32):
        return E32(np.exp(x.v))
    ev = np.exp(x.v)
    return V(ev, ev, V._rounded(ev, ev, ev * np.expm1(x.e), ELEM).e + TINY)


def log(x):
    with np.errstate(all="ignore"):
        if isinstance(x, E32):
            return E32(np.log(x.v))
        lv = np.log(x.v)
        return V._rounded(lv, np.abs(lv), -np.log1p(-x.e / x.v), ELEM)


def sqrt(x):
    if isinstance(x, E32):
        return E32(np.sqrt(x.v))
    sv = np.sqrt(x.v)
    below = sv + np.sqrt(np.maximum(x.v - x.e, 0.0))
    e = np.where(below > 0, x.e / np.where(below > 0, below, 1.0), np.sqrt(x.e))
    return V._rounded(sv, sv, e, ELEM)


def where(c, x, y):
    if isinstance(x, E32):
        return E32(np.where(c, x.v, y.v))
    return V(np.where(c, x.v, y.v), np.where(c, x.a, y.a), np.where(c, x.e, y.e))


# ------------------------------------------------------------------------------------------------------------- row reductions
class Rows:
    """which set every row is summed into (-1: none), and the slab (partial sum) it passes through on the way: slabs are
    numbered in the order they are added, `slab_set` names the set of each"""

    def __init__(self, set_, nsets, slab, slab_set):
        self.set, self.nsets, self.slab, self.slab_set = set_.astype(np.int64), int(nsets), slab.astype(np.int64), slab_set

    def drop(self, dead):
        return Rows(np.where(dead, -1, self.set), self.nsets, self.slab, self.slab_set)


def _seq(seg, nseg, rank, term, shape):
    """acc[s] = the terms of the rows with seg == s, added one after the other in ascending `rank`, in fp32"""
    rows = np.flatnonzero(seg >= 0)
    acc = np.zeros((nseg,) + tuple(shape), F32)
    if rows.size == 0:
        return acc
    o = rows[np.lexsort((rank[rows], seg[rows]))]
    s = seg[o]
    start = np.r_[0, np.flatnonzero(s[1:] != s[:-1]) + 1]
    pos = np.arange(s.size) - np.repeat(start, np.diff(np.r_[start, s.size]))
    by_pos = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[by_pos], np.arange(int(pos.max()) + 2))
    for p in range(cuts.size - 1):   # the p-th term of every segment at once
        sel = by_pos[cuts[p]:cuts[p + 1]]
        acc[s[sel]] = acc[s[sel]] + term(o[sel])
    return acc


def _emulated_rows(g, n, term, shape):
    if EMU["order"] == "chunks":
        part = _seq(np.where(g.set >= 0, g.slab, -1), g.slab_set.size, np.arange(n), term, shape)
        return _seq(g.slab_set, g.nsets, np.arange(g.slab_set.size), lambda s: part[s], shape)
    rank = np.arange(n) if EMU["order"] == "rows" else EMU["rng"].permutation(n)
    return _seq(g.set, g.nsets, rank, term, shape)


def _onehot(g, n):
    return (g.set[None, :] == np.arange(g.nsets)[:, None]).astype(F64)


def rowsum(x, g):
    """out[s, ...] = sum over the rows n of set s of x[n, ...]"""
    n = x.shape[0]
    if isinstance(x, E32):
        return E32(_emulated_rows(g, n, lambda r: x.v[r], x.shape[1:]))
    h = _onehot(g, n)
    flat = lambda a: a.reshape(n, -1)
    back = lambda a: a.reshape((g.nsets,) + x.shape[1:])
    terms = h.sum(1).reshape((g.nsets,) + (1,) * (x.v.ndim - 1))
    mag = back(h @ flat(np.abs(x.v) + x.e))
    return V(back(h @ flat(x.v)), back(h @ flat(x.a)), back(h @ flat(x.e)) + gamma(terms - 1) * mag)


def rowdot(w, x, g):
    """out[s, k, c] = sum over the rows n of set s of w[n, k] x[n, c]"""
    n, k, c = w.shape[0], w.shape[1], x.shape[1]
    if isinstance(w, E32):
        return E32(_emulated_rows(g, n, lambda r: w.v[r][:, :, None] * x.v[r][:, None, :], (k, c)))
    v, a, e = (np.zeros((g.nsets, k, c)) for _ in range(3))
    for s in range(g.nsets):
        r = g.set == s
        wv, xv, we, xe = np.abs(w.v[r]), np.abs(x.v[r]), w.e[r], x.e[r]
        mag = wv.T @ xv
        et = wv.T @ xe + we.T @ xv + we.T @ xe
        et = et + U * (mag + et)
        v[s], a[s], e[s] = w.v[r].T @ x.v[r], w.a[r].T @ x.a[r], et + gamma(int(r.sum()) - 1) * (mag + et)
    return V(v, a, e)


def rowmat(a, b, set_):
    """out[n, c] = sum_k a[n, k] b[set[n], k, c]"""
    n, k, c = a.shape[0], a.shape[1], b.shape[2]
    if isinstance(a, E32):
        acc = np.zeros((n, c), F32)
        for i in range(k):
            acc = acc + a.v[:, i, None] * b.v[set_, i, :]
        return E32(acc)
    v, m, e = (np.zeros((n, c)) for _ in range(3))
    for s in range(b.shape[0]):
        r = set_ == s
        av, bv, ae, be = np.abs(a.v[r]), np.abs(b.v[s]), a.e[r], b.e[s]
        mag = av @ bv
        et = av @ be + ae @ bv + ae @ be
        et = et + U * (mag + et)
        v[r], m[r], e[r] = a.v[r] @ b.v[s], a.a[r] @ b.a[s], et + gamma(k - 1) * (mag + et)
    return V(v, m, e)


# --------------------------------------------------------------------------------------------------------------------- pieces
def _kmap(k):
    """the `class k read as k - 64 for k >= 64` mutation"""
    i = np.arange(k)
    return np.where(i >= 64, i - 64, i)


def _lse(l):
    """rows of logits (n, K) -> (exp(l - max), their sum, max + log(sum)); the max subtraction belongs to the statement: the
    wide tier overflows without it"""
    m = l.lift(l.v.max(1, keepdims=True))   # a selection: exact
    ex = exp(l - m)
    s = ex.sum(1, keepdims=True)
    return ex, s, m + log(s)


def _softmax(l):
    ex, s, _ = _lse(l)
    return ex / s


def scene_geometry(offset, n, mode, per_scene=True):
    """Rows of the scene kernels: 256-row chunks of every scene (as many per scene as the largest needs), the sets being the
    scenes (mode 0 / per-scene prototypes) or the whole batch"""
    off = np.asarray(offset, np.int64)
    b, lo = off.size, np.r_[0, off[:-1]]
    scene = np.searchsorted(off, np.arange(n), side="right")
    pos = np.arange(n) - lo[scene]
    j = max(-(-int((off - lo).max()) // CHUNK), 1)
    sets = mode == 0 and per_scene
    g = Rows(scene if sets else np.zeros(n, np.int64), b if sets else 1, scene * j + pos // CHUNK,
             np.arange(b * j) // j if sets else np.zeros(b * j, np.int64))
    g.scene, g.pos, g.j, g.b = scene, pos, j, b
    return g


def _dropped(g, mut):
    """rows the `tile` (last row of every 16-row tile) and `slab` (last slab of every set) mutations leave out"""
    if mut == "tile":
        return g.drop(g.pos % 16 == 15)
    if mut == "slab":
        last = np.array([np.flatnonzero(g.slab_set == s).max() for s in range(g.nsets)])
        return g.drop(g.slab == last[np.maximum(g.set, 0)])
    return g


# --------------------------------------------------------------------------------------------------------------- weighted sums
def _weights(t, dt, mut):
    k = t["k"]
    if t["mode"] == 1:
        y = t["label"].astype(np.int64)
        if mut == "ign0":   # label -1 counted as class 0
            y = np.where(y == -1, 0, y)
        w = inp((y[:, None] == np.arange(k)[None, :]).astype(F32), dt)
    else:
        p = _softmax(inp(t["logits"], dt))
        top = p.v.max(1)
        keep = np.ones(top.shape, bool) if t["thr"] <= 0 else (top < t["thr"] if mut == "mask" else top >= t["thr"])
        w = p * p.lift(keep[:, None].astype(F32))
    return w[:, _kmap(k)] if mut == "k64" else w


def _wsum(t, dt, mut):
    x, w = inp(t["x"], dt), _weights(t, dt, mut)
    g = scene_geometry(t["offset"], x.shape[0], t["mode"])
    gd = _dropped(g, mut)
    if t["mode"] == 1:   # z is a count: exact
        z = inp(w.v[gd.set >= 0].astype(F64).sum(0)[None, :], dt)
    else:
        z = rowsum(w, gd)
    out = rowdot(w, x, gd) / (z + z.lift(_c(t["eps"])))[:, :, None]
    return x, w, g, z, out


def weighted_sum_forward(t, dt=F64, mut=None):
    """mode 0: w_nk = softmax(logits_n)_k [max_k p_nk >= thr] (thr <= 0: no mask), per scene; mode 1: w_nk = [label_n == k], one
    set.  z = sum_n w_nk, out = sum_n w_nk x_n / (z + eps)"""
    _, _, _, z, out = _wsum(t, dt, mut)
    return dict(z=z.v.copy() if t["mode"] == 1 else z, out=out)


def weighted_sum_backward(t, dt=F64, mut=None):
    """gx_n = sum_k w_nk / (z_k + eps) dout_k; glogits_nj = w_nj (dw_nj - sum_k w_nk dw_nk), dw_nk = (<x_n, dout_k> -
    <out_k, dout_k>) / (z_k + eps): the gradient through the softmax with the mask held constant.  z and out are the forward's"""
    x, w, g, z, out = _wsum(t, dt, mut if mut in ("k64", "mask", "ign0") else None)
    dout = inp(t["dout"], dt)
    zinv = (z.lift(F32(1.0)) / (z + z.lift(_c(t["eps"]))))[g.set]
    res = dict(gx=rowmat(w * zinv, dout, g.set))
    if t["mode"] == 0 and t.get("glogits", True):
        dw = (rowmat(x, dout.t(), g.set) - (out * dout).sum(2)[g.set]) * zinv
        res["glogits"] = w * (dw - (w * dw).sum(1, keepdims=True))
    return res


# ---------------------------------------------------------------------------------------------------------------------- cosine
def _normalise(x, mut=None):
    """rows x (..., C) -> (x / max(|x|, 1e-12), |x|); the `sq` mutation divides by |x|^2"""
    ss = (x * x).sum(-1, keepdims=True)
    nr = sqrt(ss)
    den = ss if mut == "sq" else nr
    return x / where(den.v > _c(1e-12), den, den.lift(np.full(den.shape, _c(1e-12)))), nr


def _cos(t, dt, mut):
    x, q = inp(t["x"], dt), inp(t["q"].reshape((-1,) + t["q"].shape[-2:]), dt)
    g = scene_geometry(t["offset"], x.shape[0], 0, bool(t["per_scene"]))
    xh, xn = _normalise(x, mut)
    qh, qn = _normalise(q)
    return x, q, g, xh, xn, qh, qn


def cosine_forward(t, dt=F64, mut=None):
    """out_nk = scale <x_n / max(|x_n|, 1e-12), q_k / max(|q_k|, 1e-12)>, q of the row's scene or shared"""
    x, q, g, xh, _, qh, _ = _cos(t, dt, mut)
    if mut == "k64":
        qh = qh[:, _kmap(t["k"])]
    return dict(out=rowmat(xh, qh.t(), g.set) * xh.lift(_c(t["scale"])))


def _through_norm(d, h, nr):
    """the gradient d of h = v / max(|v|, eps) taken back to v: (d - h <h, d>) / |v| above the clamp, d / eps below"""
    big = nr.v > _c(1e-12)
    safe = where(big, nr, nr.lift(np.ones(nr.shape)))
    return where(big, (d - h * (h * d).sum(-1, keepdims=True)) / safe, d / d.lift(_c(1e-12)))


def cosine_backward(t, dt=F64, mut=None):
    """gx and gq of out = scale <xhat, qhat> for the upstream gradient dout (N, K)"""
    x, q, g, xh, xn, qh, qn = _cos(t, dt, mut if mut == "sq" else None)
    gs = inp(t["dout"], dt) * xh.lift(_c(t["scale"]))
    gx = _through_norm(rowmat(gs, qh, g.set), xh, xn)
    gq = _through_norm(rowdot(gs, xh, _dropped(g, mut)), qh, qn)
    return dict(gx=gx, gq=gq.reshape(t["q"].shape))


# ---------------------------------------------------------------------------------------------------------------- distillation
def _distill(t, dt, mut):
    pred, soft, y = inp(t["pred"], dt), inp(t["soft"], dt), t["label"].astype(np.int64)
    n, k = pred.shape
    if mut == "k64":
        pred = pred[:, _kmap(k)]
    _, _, lse = _lse(pred)
    sm = _softmax(soft)
    valid = y != -1
    hot = np.where(valid, y, 0)
    half = sm.lift(F32(0.5))
    target = sm * half + sm.lift((hot[:, None] == np.arange(k)[None, :]).astype(F32)) * half
    loss = -((pred - lse) * target).sum(1)
    ent = -(sm * log(sm + sm.lift(_c(1e-4)))).sum(1)
    weighted = valid | (mut == "ent1")   # the mutation: an ignored row's one-hot class 0 with entropy weight 1
    ent = ent * ent.lift(weighted.astype(F32))
    cls = np.where(weighted, hot, -1)
    chunk = np.arange(n) // CHUNK
    g = Rows(cls, k, chunk * k + np.maximum(cls, 0), np.arange((int(chunk.max()) + 1) * k) % k)
    if mut == "slab":
        g = g.drop(chunk == chunk.max())
    return pred, lse, target, loss, ent, g, cls


def distill_forward(t, dt=F64, mut=None):
    """get_distill_loss(pred, soft, label, smoothness 0.5, eps 0): loss_n = -<log_softmax(pred_n), 0.5 softmax(soft_n) + 0.5
    onehot(label_n)> (an ignored row's one-hot on class 0), ent_n = -<sm_n, log(sm_n + 1e-4)> (0 for an ignored row);
    loss = sum over the present classes of (sum_n loss_n ent_n) / (sum_n ent_n + 1e-4), over (present + 1e-4);
    coef_k = d loss / d (loss_n ent_n) of a row of class k; rows = the labelled rows per class"""
    pred, lse, target, loss_n, ent, g, cls = _distill(t, dt, mut)
    k = pred.shape[1]
    rows = np.bincount(g.set[g.set >= 0], minlength=k).astype(F64)
    num, den = rowsum(loss_n * ent, g), rowsum(ent, g)
    present = rows > 0
    pc = num.lift(F32(present.sum())) + num.lift(_c(1e-4))
    dplus = where(present, den + den.lift(_c(1e-4)), den.lift(np.ones(k)))
    zero = num.lift(np.zeros(k))
    loss = where(present, num / dplus, zero).sum(0) / pc
    coef = where(present, num.lift(np.ones(k)) / dplus / pc, zero)
    return dict(loss=loss.reshape(1), coef=coef, rows=rows)


def distill_backward(t, dt=F64, mut=None):
    """gpred_n = g ent_n coef_{label_n} (softmax(pred_n) sum_k target_nk - target_n), zero for an ignored row; coef is the
    forward's"""
    pred, lse, target, _, ent, g, cls = _distill(t, dt, mut)
    coef = distill_forward(t, dt, mut)["coef"]
    f = ent * coef[np.maximum(cls, 0)] * ent.lift(_c(t["g"])) * ent.lift((cls >= 0).astype(F32))
    gp = (exp(pred - lse) * target.sum(1, keepdims=True) - target) * f.reshape(-1, 1)
    if dt is F64:   # an ignored row is zero, exactly
        dead = (cls < 0)[:, None]
        gp = V(np.where(dead, 0.0, gp.v), np.where(dead, 0.0, gp.a), np.where(dead, 0.0, gp.e))
    return dict(gpred=gp)


# --------------------------------------------------------------------------------------------------------------- cross-entropy
def _ce(t, dt):
    logits, y, c = inp(t["logits"], dt), t["label"].astype(np.int64), t["logits"].shape[1]
    live = y != t["ignore_index"]
    on = live & (y >= 0) & (y < c)
    return logits, y, on, int((live & ~on).sum()), _lse(logits)[2].reshape(-1)


def cross_entropy_forward(t, dt=F64, mut=None):
    """lse_n; loss = mean over the labelled rows of lse_n - logits[n, label_n]; count = the labelled rows; bad_labels = labels
    that are neither ignore_index nor in [0, c), which make the loss nan, as does count == 0"""
    logits, y, on, bad, lse = _ce(t, dt)
    n = y.size
    count = n if mut == "mean_n" else int(on.sum())
    res = dict(lse=lse, count=np.array([on.sum()], F64), bad_labels=np.array([bad], F64))
    if bad or not on.any():
        res["loss"] = np.array([np.nan])
        return res
    g = Rows(np.where(on, 0, -1), 1, np.arange(n) // CHUNK, np.zeros(-(-n // CHUNK), np.int64))
    picked = logits[np.arange(n), np.where(on, y, 0)]
    res["loss"] = rowsum(lse - picked, g) / lse.lift(F32(count))
    return res


def cross_entropy_backward(t, dt=F64, mut=None):
    """g_logits = (softmax(logits_n) - onehot(label_n)) g / count for a labelled row, zero for the others and when no row is
    labelled; lse is the forward's"""
    logits, y, on, bad, lse = _ce(t, dt)
    n, c = logits.shape
    count = n if mut == "mean_n" else int(on.sum())
    zero = logits.lift(np.zeros((n, c)))
    if count == 0:
        return dict(g_logits=zero)
    scale = logits.lift(_c(t["g"])) / logits.lift(F32(count))
    hot = logits.lift((y[:, None] == np.arange(c)[None, :]).astype(F32))
    return dict(g_logits=where(on[:, None], (exp(logits - lse.reshape(-1, 1)) - hot) * scale, zero))


CONTRACTS = dict(
    cac_weighted_sum_forward_hip_launcher=weighted_sum_forward,
    cac_weighted_sum_backward_hip_launcher=weighted_sum_backward,
    cac_cosine_forward_hip_launcher=cosine_forward,
    cac_cosine_backward_hip_launcher=cosine_backward,
    cac_distill_forward_hip_launcher=distill_forward,
    cac_distill_backward_hip_launcher=distill_backward,
    cross_entropy_forward_hip_launcher=cross_entropy_forward,
    cross_entropy_backward_hip_launcher=cross_entropy_backward,
)

# the outputs compared for every launcher (asserted against what a run returns; glogits when the case asks for it)
KEYS = dict(
    cac_weighted_sum_forward_hip_launcher=("z", "out"),
    cac_weighted_sum_backward_hip_launcher=("gx", "glogits"),
    cac_cosine_forward_hip_launcher=("out",),
    cac_cosine_backward_hip_launcher=("gx", "gq"),
    cac_distill_forward_hip_launcher=("loss", "coef", "rows"),
    cac_distill_backward_hip_launcher=("gpred",),
    cross_entropy_forward_hip_launcher=("lse", "loss", "count", "bad_labels"),
    cross_entropy_backward_hip_launcher=("g_logits",),
)

# the deliberately wrong variants of every contract (tests/test_cac_ref64_host.py)
MUTANTS = dict(
    cac_weighted_sum_forward_hip_launcher=("tile", "slab", "k64", "mask", "ign0"),
    cac_weighted_sum_backward_hip_launcher=("k64", "mask", "ign0"),
    cac_cosine_forward_hip_launcher=("k64", "sq"),
    cac_cosine_backward_hip_launcher=("tile", "slab", "sq"),
    cac_distill_forward_hip_launcher=("slab", "k64", "ent1"),
    cac_distill_backward_hip_launcher=("k64", "ent1"),
    cross_entropy_forward_hip_launcher=("mean_n",),
    cross_entropy_backward_hip_launcher=("mean_n",),
)


def emulate(fn, t, order, rng=None, mut=None):
    """the fp32 emulation of statement `fn` with its row sums in `order`: {output name: fp32 / exact array}"""
    EMU.update(order=order, rng=rng)
    try:
        return {k: (o.v if isinstance(o, E32) else o) for k, o in fn(t, F32, mut).items()}
    finally:
        EMU.update(order="rows", rng=None)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32)[~np.isnan(a)], b.view(np.int32)[~np.isnan(b)])) \
        and bool(np.array_equal(np.isnan(a), np.isnan(b)))


def compare(got, ref):
    """(ok, worst err / bound, message) of one output: `got` the fp32 array under test, `ref` the float64 statement's V (the
    bound per element; where the bound is 0 the value is exact) or a plain array (bit equality with its fp32 rounding)"""
    got = np.ascontiguousarray(got)
    if not isinstance(ref, V):
        want = np.asarray(ref).astype(F32)
        if got.shape != want.shape:
            return False, float("inf"), "shape %s, expected %s" % (got.shape, want.shape)
        ok = bits_equal(got, want)
        return ok, 0.0 if ok else float("inf"), "" if ok else "got %r, expected %r" % (got.ravel()[:8], want.ravel()[:8])
    if got.shape != ref.v.shape:
        return False, float("inf"), "shape %s, expected %s" % (got.shape, ref.v.shape)
    if not np.isfinite(got).all():
        return False, float("inf"), "not finite (an unwritten element shows as NaN)"
    assert np.isfinite(ref.e).all() and np.isfinite(ref.v).all(), "the reference's own bound is not finite"
    err = np.abs(got.astype(F64) - ref.v)
    bad = err > ref.e
    ratio = float((err[ref.e > 0] / ref.e[ref.e > 0]).max()) if (ref.e > 0).any() else 0.0
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        return False, max(ratio, 1.0), "%d elements out of bound, first flat index %d: got %r, float64 %r, A %r, bound %r" % (
            int(bad.sum()), i, float(got.ravel()[i]), float(ref.v.ravel()[i]), float(ref.a.ravel()[i]), float(ref.e.ravel()[i]))
    return True, ratio, ""
