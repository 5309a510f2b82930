"""The inputs of tests/test_gpu_gather_f64.py and tests/test_gather_ref64_host.py: for every launcher of
ao_amd/csrc/gather_ops.hip and ao_amd/csrc/pool.hip a list of small cases, each in two value tiers.

exact     operands are non-zero multiples of 2^-bits in [-2, 2] (bits = 3, fewer where an output collects very many terms: the builder
          takes the largest bits <= 3 for which, with f the fractional bits of a term, A 2^f is an integer below 2^24 for every
          output element -- asserted on the float64 side by `check_exact`).  Every term and every partial sum in any order is
          then representable in fp32: the kernel must return float32(value) bit for bit.
rounding  operands are standard normal with |x| >= 2^-6, so no |term| is below 2^-20 (`check_rounding`).

Shapes: channels 1, 3, 4, 6, 48, 50 (scalar and float4 forms) and 48 on a base pointer one float off a 16-byte boundary (flag
`offset`: the GPU test places every float array at buf[1:]); rows 0, 1, 257, 1500; neighbour counts 1, 3, 8, 9, 16; inverse
lists and clusters of 0 (lists only), 1, 2, 8, 9, 10, 17, 18 entries planted on rows 0 ... 7; every row aimed at one target
(`contention`); one `big` case per launcher whose thread count is just above the launcher's grid cap x 256, so that the
grid-stride loop takes its second trip (exact tier only).  No index is negative or out of range except where the launcher
guards it (grouping: -1; interpolation_weights: -1 is rewritten).  No NaN / Inf.  A cluster has at least one member."""
import collections
import zlib

import numpy as np

from tests import gather_ref64 as R

F32 = np.float32
TIERS = ("exact", "rounding")
PLANTED = (0, 1, 2, 8, 9, 10, 17, 18)            # inverse-list lengths of rows 0 ... 7
CLUSTER_LENGTHS = (1, 2, 8, 9, 10, 17, 18)       # cycled over the first clusters
GRID_CAP = dict(default=2048, segment_sum_hip_launcher=4096)

Case = collections.namedtuple("Case", "launcher name p flags")


def _case(launcher, name, flags=(), **p):
    return Case(launcher, name, p, frozenset(flags))


def second_trip_threads(launcher):
    return GRID_CAP.get(launcher, GRID_CAP["default"]) * 256


# ------------------------------------------------------------------------------------------------------------------ case list
# (rows, neighbours, channels[, flags]) of the neighbour-table ops
NEIGH = [(0, 3, 4), (1, 1, 1), (1, 16, 3), (257, 3, 4), (257, 8, 6), (257, 9, 48), (257, 16, 50), (257, 16, 48, "offset"),
         (1500, 1, 48), (1500, 3, 6)]
# (edges m, groups g, channels c, points n[, flags]) of the attention steps; index_target is unsorted with duplicates unless
# flagged `sorted`
EDGES = [(0, 1, 4, 5), (1, 1, 1, 1), (257, 1, 3, 40), (257, 6, 4, 40), (257, 6, 48, 20), (257, 1, 50, 40), (1500, 1, 6, 200),
         (257, 6, 8, 40, "offset"), (257, 6, 8, 40, "sorted"), (257, 6, 8, 40, "contention")]
# (clusters, channels[, flags]) of the pooling ops
POOL = [(1, 1), (1, 4), (257, 3), (257, 4), (257, 6), (257, 48), (257, 50), (257, 48, "offset"), (1500, 4), (1500, 1),
        (257, 4, "ties"), (257, 6, "ties"), (257, 48, "ties"), (257, 48, "ties", "offset")]


def _name(*parts):
    return "-".join(str(p) for p in parts if p != "")


def _neigh_cases(launcher, extra=(), contention=False, big=None):
    out = []
    for rows, ns, c, *flags in NEIGH:
        out.append(_case(launcher, _name("r%d" % rows, "s%d" % ns, "c%d" % c, *flags), flags, rows=rows, ns=ns, c=c))
    if contention:
        out.append(_case(launcher, "r257-s8-c6-contention", ("contention",), rows=257, ns=8, c=6))
    out.extend(extra)
    if big:
        out.append(_case(launcher, _name("r%d" % big[0], "s%d" % big[1], "c%d" % big[2], "big"), ("big",), rows=big[0], ns=big[1],
                         c=big[2], **(big[3] if len(big) > 3 else {})))
    return out


def _edge_cases(launcher, big):
    out = [_case(launcher, _name("m%d" % m, "g%d" % g, "c%d" % c, *flags), flags, m=m, g=g, c=c, n=n)
           for m, g, c, n, *flags in EDGES]
    out.append(_case(launcher, _name("m%d" % big[0], "g%d" % big[1], "c%d" % big[2], "big"), ("big",), m=big[0], g=big[1], c=big[2],
                     n=64))
    return out


def _pool_cases(launcher, big):
    out = [_case(launcher, _name("j%d" % j, "c%d" % c, *flags), flags, n_out=j, c=c) for j, c, *flags in POOL
           if launcher == "pool_max_forward_hip_launcher" or "ties" not in flags]
    out.append(_case(launcher, _name("j%d" % big[0], "c%d" % big[1], "big"), ("big",), n_out=big[0], c=big[1]))
    return out


def _aggregation_cases(launcher):
    extra = [_case(launcher, "r257-s8-c48-w%d" % w, (), rows=257, ns=8, c=48, w_c=w) for w in (1, 6, 48, 5)]
    extra.append(_case(launcher, "r257-s8-c6-w4", (), rows=257, ns=8, c=6, w_c=4))
    return _neigh_cases(launcher, extra, contention=launcher.startswith("aggregation_backward"), big=(16400, 2, 32, dict(w_c=4)))


CASES = collections.OrderedDict()
CASES["grouping_forward_hip_launcher"] = _neigh_cases("grouping_forward_hip_launcher", big=(4099, 16, 32))
CASES["grouping_backward_hip_launcher"] = _neigh_cases("grouping_backward_hip_launcher", contention=True, big=(4099, 16, 8))
CASES["interpolation_weights_hip_launcher"] = (
    [_case("interpolation_weights_hip_launcher", "m%d-k%d" % (m, k), (), rows=m, ns=k) for m, k in
     [(0, 3), (1, 1), (257, 1), (257, 2), (257, 3), (257, 4), (257, 5), (257, 6), (257, 7), (257, 8), (1500, 3)]]
    + [_case("interpolation_weights_hip_launcher", "m524300-k2-big", ("big",), rows=524300, ns=2)])
CASES["interpolation_forward_hip_launcher"] = _neigh_cases("interpolation_forward_hip_launcher", big=(16400, 3, 32))
CASES["interpolation_backward_hip_launcher"] = _neigh_cases("interpolation_backward_hip_launcher", contention=True,
                                                            big=(16400, 3, 32))
CASES["interpolation_backward_gather_hip_launcher"] = _neigh_cases(
    "interpolation_backward_gather_hip_launcher", contention=True, big=(16390, 2, 128),
    extra=[_case("interpolation_backward_gather_hip_launcher", "r257-s1-c%d-ones" % c, ("ones",), rows=257, ns=1, c=c) for c in (6, 48)]
    + [_case("interpolation_backward_gather_hip_launcher", "r257-s3-c%d-m257" % c, ("square",), rows=257, ns=3, c=c) for c in (4, 50)])
CASES["subtraction_forward_hip_launcher"] = _neigh_cases("subtraction_forward_hip_launcher", big=(4099, 16, 32))
CASES["subtraction_backward_hip_launcher"] = _neigh_cases("subtraction_backward_hip_launcher", contention=True, big=(16400, 2, 32))
CASES["aggregation_forward_hip_launcher"] = _aggregation_cases("aggregation_forward_hip_launcher")
CASES["aggregation_backward_hip_launcher"] = _aggregation_cases("aggregation_backward_hip_launcher")
CASES["attention_relation_step_forward_hip_launcher"] = _edge_cases("attention_relation_step_forward_hip_launcher", (87400, 6, 4))
CASES["attention_relation_step_backward_hip_launcher"] = _edge_cases("attention_relation_step_backward_hip_launcher", (21850, 6, 4))
CASES["attention_fusion_step_forward_hip_launcher"] = _edge_cases("attention_fusion_step_forward_hip_launcher", (21850, 6, 4))
CASES["attention_fusion_step_backward_hip_launcher"] = _edge_cases("attention_fusion_step_backward_hip_launcher", (87400, 6, 4))
CASES["segment_minmax_hip_launcher"] = [
    _case("segment_minmax_hip_launcher", _name("b%d" % len(sizes), "n%d" % sum(sizes), sign), (), sizes=sizes, sign=sign)
    for sizes in ((1,), (300,), (1, 300, 20000), (20000, 1, 63)) for sign in ("mixed", "positive", "negative")]
CASES["pool_max_forward_hip_launcher"] = _pool_cases("pool_max_forward_hip_launcher", (65540, 32))
CASES["pool_max_backward_hip_launcher"] = _pool_cases("pool_max_backward_hip_launcher", (16400, 32))
CASES["segment_sum_hip_launcher"] = _pool_cases("segment_sum_hip_launcher", (31776, 33))


def threads(case):
    """the launcher's `total`: how many grid-stride iterations the launch is made of (the vector forms count float4 lanes)"""
    p, name = case.p, case.launcher
    vec = lambda c: c // 4 if c % 4 == 0 and "offset" not in case.flags else c
    if name in ("grouping_forward_hip_launcher", "subtraction_forward_hip_launcher"):
        return p["rows"] * p["ns"] * vec(p["c"])
    if name == "grouping_backward_hip_launcher":
        return p["rows"] * p["ns"] * p["c"]
    if name == "interpolation_weights_hip_launcher":
        return p["rows"]
    if name == "interpolation_backward_gather_hip_launcher":
        return source_rows(case) * vec(p["c"])
    if name in ("attention_relation_step_forward_hip_launcher", "attention_fusion_step_backward_hip_launcher"):
        return p["m"] * p["g"]
    if name.startswith("attention_"):
        return p["m"] * p["g"] * p["c"]
    if name in ("pool_max_forward_hip_launcher", "segment_sum_hip_launcher"):
        return p["n_out"] * vec(p["c"])
    if name == "pool_max_backward_hip_launcher":
        return p["n_out"] * p["c"]
    if name == "segment_minmax_hip_launcher":
        return max(p["sizes"])
    return p["rows"] * p["c"]


def tiers(case):
    if "big" in case.flags:
        return ("exact",)
    if case.launcher == "interpolation_weights_hip_launcher" and case.p["ns"] not in (1, 2, 4):
        return ("rounding",)   # the weights' exact tier (equal distances: every weight 1 / k) needs k r exact in slot order
    return TIERS


def pairs(launcher):
    return [(case, tier) for case in CASES[launcher] for tier in tiers(case)]


# ------------------------------------------------------------------------------------------------------------------- builders
def _rng(case, tier, bits):
    # the gather form of the interpolation backward runs on the idx, weights and gradients of the atomic form's cases
    launcher = case.launcher.replace("_backward_gather_", "_backward_")
    return np.random.default_rng(zlib.crc32(("%s/%s/%s/%d" % (launcher, case.name, tier, bits)).encode()))


def _values(rng, shape, tier, bits):
    if tier == "exact":
        k = rng.integers(1, (2 << bits) + 1, shape) * np.where(rng.random(shape) < 0.5, -1, 1)   # no zeros: every term counts
        return (k / float(1 << bits)).astype(F32)
    x = rng.standard_normal(shape).astype(F32)
    small = np.abs(x) < 2.0 ** -6
    x[small] = np.where(x[small] < 0, -1, 1) * F32(2.0 ** -6)
    return x


def _index(rng, slots, n, contention=False):
    """`slots` ids in [0, n).  With room for it, rows 0 ... 7 are aimed at exactly PLANTED times (row 0: by nobody)"""
    if contention:
        return np.full(slots, min(3, n - 1), np.int32)
    planted = int(sum(PLANTED))
    if slots < planted or n < 10:
        return rng.integers(0, max(n, 1), slots).astype(np.int32)
    ids = np.r_[np.repeat(np.arange(8), PLANTED), rng.integers(8, n, slots - planted)]
    return rng.permutation(ids).astype(np.int32)


def source_rows(case):
    """how many rows the index of a neighbour-table case points into"""
    rows, name = case.p["rows"], case.launcher
    if name.startswith(("subtraction", "aggregation")):
        return max(rows, 1)                       # input2 / input have the rows of the table
    if "square" in case.flags or (name == "interpolation_backward_gather_hip_launcher" and "big" in case.flags):
        return rows                                # m == n, the largest the gather form takes
    return max(10, rows // 3) if rows > 1 else 1   # grouping: n points; interpolation: the coarse cloud, m < n


def _clusters(rng, n_out):
    length = np.array([CLUSTER_LENGTHS[j % len(CLUSTER_LENGTHS)] if j < 21 else rng.integers(1, 21) for j in range(n_out)])
    if n_out > 40000:
        length = rng.integers(1, 3, n_out)       # the second-trip case: many short clusters
    n_in = int(length.sum())
    return length, rng.permutation(n_in).astype(np.int32), np.r_[0, np.cumsum(length)].astype(np.int32), n_in


def _plant_ties(feat, order, ptr):
    """clusters whose maximum occurs twice (first and a later member; members 9 and 10, across the unroll of 8 behind the first
    member), an all-equal cluster, a negative-only cluster, -0.0 against +0.0 in both orders"""
    length = np.diff(ptr)
    first = lambda n, skip=0: int(np.flatnonzero(length == n)[skip])
    member = lambda j, i: order[ptr[j] + i]
    top = F32(3.0)                                             # above every other value of either tier
    a, b, c9, d, e, f, g = first(17), first(18), first(9), first(8), first(2), first(2, 1), first(10)
    feat[member(a, 0)] = feat[member(a, 5)] = top
    feat[member(b, 8)] = feat[member(b, 9)] = top
    feat[order[ptr[c9]:ptr[c9 + 1]]] = F32(0.5)
    rows = order[ptr[d]:ptr[d + 1]]
    feat[rows] = -np.abs(feat[rows]) - F32(0.125)
    feat[member(e, 0)], feat[member(e, 1)] = F32(-0.0), F32(0.0)
    feat[member(f, 0)], feat[member(f, 1)] = F32(0.0), F32(-0.0)
    rows = order[ptr[g]:ptr[g + 1]]
    feat[rows] = -np.abs(feat[rows]) - F32(0.125)
    feat[member(g, 0)], feat[member(g, 9)] = F32(-0.0), F32(0.0)
    # a second 17-cluster: the maximum at members 1, 8 and 16 (inside the first batch of 8, its last slot, the last member)
    h = first(17, 1)
    feat[member(h, 1)] = feat[member(h, 8)] = feat[member(h, 16)] = top


def _build(case, tier, bits):
    rng = _rng(case, tier, bits)
    v = lambda *shape: _values(rng, shape, tier, bits)
    p, name, flags = case.p, case.launcher, case.flags
    if name == "segment_minmax_hip_launcher":
        xyz = v(sum(p["sizes"]), 3)
        if p["sign"] != "mixed":
            xyz = (np.abs(xyz) + F32(0.125)) * F32(1 if p["sign"] == "positive" else -1)
        ends = np.cumsum(p["sizes"]) - 1          # the last point of a cloud holds its maximum in x and its minimum in z
        xyz[ends, 0] = np.abs(xyz).max() + 1 if p["sign"] != "negative" else F32(-0.0625)
        xyz[ends, 2] = -np.abs(xyz).max() - 1 if p["sign"] != "positive" else F32(0.0625)
        return dict(xyz=xyz, offset=np.cumsum(p["sizes"]).astype(np.int32))
    if name in ("pool_max_forward_hip_launcher", "pool_max_backward_hip_launcher", "segment_sum_hip_launcher"):
        _, order, ptr, n_in = _clusters(rng, p["n_out"])
        if name == "segment_sum_hip_launcher":
            return dict(grad_fine=v(n_in, p["c"]), order=order, idx_ptr=ptr)
        feat = v(n_in, p["c"])
        if "ties" in flags:
            _plant_ties(feat, order, ptr)
        t = dict(feat=feat, order=order, idx_ptr=ptr)
        if name == "pool_max_backward_hip_launcher":   # arg: the reference's, of a forward on these clusters
            return dict(grad_out=v(p["n_out"], p["c"]), arg=R.pool_max_forward(t)["arg"], n_in=n_in)
        return t
    if name.startswith("attention_"):
        m, g, c, n = p["m"], p["g"], p["c"], p["n"]
        tgt = _index(rng, m, n, "contention" in flags)
        if "sorted" in flags:
            tgt = np.sort(tgt)
        t = dict(index_target=tgt, index_refer=_index(rng, m, n))
        if "relation" in name:
            t.update(query=v(n, g, c), key=v(n, g, c), weight=v(c))
            if "backward" in name:
                t["grad_output"] = v(m, g)
        else:
            t.update(weight=v(m, g), value=v(n, g, c))
            if "backward" in name:
                t["grad_output"] = v(n, g, c)
        return t
    rows, ns = p["rows"], p["ns"]
    if name == "interpolation_weights_hip_launcher":
        n = 50
        idx = rng.integers(0, n, (rows, ns)).astype(np.int32)
        idx[rng.random((rows, ns)) < 0.1] = -1                       # a coarse segment shorter than k
        if tier == "exact":   # all distances of a row equal and k a power of two: every weight is 1 / k exactly
            d2 = np.repeat(np.abs(_values(rng, (rows, 1), "exact", 3)), ns, axis=1)
        else:
            d2 = _values(rng, (rows, ns), tier, bits) ** 2
            if rows > 4:
                d2[1, ns // 2] = 0            # one neighbour at distance 0
                d2[3, :] = 0                  # all of them
        return dict(dist2=np.ascontiguousarray(d2, F32), idx=idx, n=n)
    c, n = p["c"], source_rows(case)
    idx = _index(rng, rows * ns, n, "contention" in flags).reshape(rows, ns)
    if name.startswith("grouping"):
        keep = idx[:1, -1].copy()
        idx[rng.random(idx.shape) < 0.1] = -1                        # guarded by the kernels: zeros / no contribution
        idx[:1, -1] = keep                                           # (the first row keeps its last neighbour)
        if name == "grouping_forward_hip_launcher":
            return dict(input=v(n, c), idx=idx)
        return dict(grad_output=v(rows, ns, c), idx=idx, n=n)
    if name.startswith("interpolation"):
        weight = np.ones((rows, ns), F32) if "ones" in flags else v(rows, ns)
        if name == "interpolation_forward_hip_launcher":
            return dict(input=v(n, c), idx=idx, weight=weight)
        return dict(grad_output=v(rows, c), idx=idx, weight=weight, m=n)
    if name == "subtraction_forward_hip_launcher":
        return dict(input1=v(rows, c), input2=v(n, c), idx=idx)
    if name == "subtraction_backward_hip_launcher":
        return dict(grad_output=v(rows, ns, c), idx=idx)
    w_c = p.get("w_c", c if c < 8 else max(c // 8, 1))
    t = dict(input=v(n, c), position=v(rows, ns, c), weight=v(rows, ns, w_c), idx=idx)
    if rows:   # input + position is a factor of every term: keep the sum away from a cancellation (exact tier: from zero)
        s = t["input"][idx] + t["position"]
        if tier == "rounding":
            t["position"] = np.where(np.abs(s) < 2.0 ** -6, t["position"] + F32(1), t["position"]).astype(F32)
        else:
            t["position"] = np.where(s == 0, t["input"][idx], t["position"]).astype(F32)
    if name == "aggregation_backward_hip_launcher":
        t["grad_output"] = v(rows, c)
    return t


def check_exact(out, bits):
    """every Sum of a float64 statement: A 2^f is an integer below 2^24 (f = factors x bits), per element"""
    for key, o in out.items():
        if isinstance(o, R.Sum):
            scaled = o.A * 2.0 ** (o.factors * bits)
            if not (np.array_equal(scaled, np.round(scaled)) and (scaled < 2.0 ** 24).all()):
                return False
    return True


def check_rounding(out):
    """no |term| below 2^-20 other than exact zeros"""
    for key, o in out.items():
        if isinstance(o, R.Sum) and o.term.size:
            a = np.abs(o.term[o.term != 0])
            if a.size and a.min() < 2.0 ** -20:
                return False
    return True


_CACHE = collections.OrderedDict()


def inputs(case, tier):
    """(inputs, float64 statement, bits) of a case in a tier, built once"""
    key = (case.launcher, case.name, tier)
    if key not in _CACHE:
        fn = R.CONTRACTS[case.launcher]
        if tier == "exact":
            for bits in (3, 2, 1, 0):
                t = _build(case, tier, bits)
                ref = fn(t)
                if check_exact(ref, bits):
                    break
            else:
                raise AssertionError("%s %s: no operand grid keeps the sums exact in fp32" % (case.launcher, case.name))
        else:
            bits = -1
            t = _build(case, tier, bits)
            ref = fn(t)
            assert check_rounding(ref), "%s %s: a term in the denormal neighbourhood" % (case.launcher, case.name)
        while len(_CACHE) >= 4:
            _CACHE.popitem(last=False)
        _CACHE[key] = (t, ref, bits)
    return _CACHE[key]
