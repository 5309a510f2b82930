"""Float64 reference of the PT-v2m2 Block and model for tests/test_gpu_ptv2_f64.py and tests/test_ptv2_ref64_host.py: plain
torch, no project kernel, runs on any device.

The Block is oracle.ptv2_ref._block itself on `dtype` copies of the state, x and coord.  The model is the statement sequence of
oracle.ptv2_ref.forward with every table passed in (per-level kNN tables, cluster / order / idx_ptr, up_idx / up_weight) instead
of built, so that the reference and the runtime under test see the same geometry.  Both run under `recording`, which hands
every ReLU pre-activation and every pooling to a Recorder: a float32 run and a float64 run that disagree on the sign of one
pre-activation, or on one pooling arg-max, differ by a whole gradient term, so the cases carry seeds with a margin (`margin`).

The float64 run is made on the device under test; the eager float32 run, the yardstick of the bound and of the margin, on the
host (`eager_host`).

F.batch_norm does not advance num_batches_tracked; nn.BatchNorm1d does, once per training forward.  The runs here add that step
to the returned buffers."""
import contextlib

import torch
import torch.nn.functional as TF

from oracle import ptv2_ref as M

FLOOR = 2.0 ** -24
RATIO = 4.0   # the margin condition: smallest |pre-activation| and pooling gap >= RATIO * largest |p32 - p64|
M_CAP = 64    # no class of output may need more than this multiple of the eager float32 run's own error


# ------------------------------------------------------------------------------------------------------------ recorder ----
class Recorder:
    """pre: every ReLU pre-activation in call order.  pools: per pooling, the gap between the two largest members of every
    (cluster, channel) with at least two members (inf where there is one member, or where the two largest are exactly 0 / 0:
    the ReLU in front has derivative 0 there, so the choice of row carries no gradient), and the rows of the two."""

    def __init__(self):
        self.pre, self.pools = [], []

    def relu(self, x):
        self.pre.append(x.detach().clone())
        return TF.relu(x)

    def pool(self, d, order, idx_ptr):
        d = d.detach()
        order, idx_ptr = order.long(), idx_ptr.long()
        counts = torch.diff(idx_ptr)
        m, c, width = counts.numel(), d.shape[1], max(int(counts.max()), 2)
        seg = torch.repeat_interleave(torch.arange(m, device=d.device), counts)
        pos = torch.arange(order.numel(), device=d.device) - idx_ptr[:-1][seg]
        pad = torch.full((m, width, c), float("-inf"), dtype=d.dtype, device=d.device)
        pad[seg, pos] = d[order]
        top, arg = pad.topk(2, dim=1)
        gap = top[:, 0] - top[:, 1]                                   # (inf for a cluster of one member)
        gap[(top[:, 0] == 0) & (top[:, 1] == 0)] = float("inf")
        rows = order[(idx_ptr[:-1].view(m, 1, 1) + arg).clamp(max=order.numel() - 1)]
        self.pools.append(dict(gap=gap, first=rows[:, 0], second=rows[:, 1]))


class _Shim:
    """torch.nn.functional with a recording relu, put in the oracle's place of `F` while a reference run is recorded"""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(TF, name)

    def relu(self, x, inplace=False):
        return self._rec.relu(x)


@contextlib.contextmanager
def recording(rec):
    old = M.F
    M.F = _Shim(rec)
    try:
        yield rec
    finally:
        M.F = old


def margin(rec64, rec32):
    """(smallest non-zero |pre-activation| and pooling gap of the float64 run, largest |p32 - p64|)"""
    assert len(rec64.pre) == len(rec32.pre) and len(rec64.pools) == len(rec32.pools)
    eps = max(float((a.double() - b).abs().max()) for a, b in zip(rec32.pre, rec64.pre))
    small = min(float(p[p != 0].abs().min()) for p in rec64.pre if bool((p != 0).any()))
    gaps = [float(p["gap"].min()) for p in rec64.pools]
    return min([small] + gaps), eps


@contextlib.contextmanager
def _own_batch_norm():
    """On the device F.batch_norm may hand a training-mode call to the vendor library; the reference takes torch's own kernels"""
    old = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = old


@contextlib.contextmanager
def eager_host():
    """The eager float32 run is the yardstick of the bound and of the margin, so it has to be the same run wherever the tests
    run: on the CPU, on one thread (its sums then run in one order).  On the MI355X torch's float32 training-mode BatchNorm
    is no such yardstick: through the vendor library the pre-activations lie 1.5e-3 from the float64 run, through torch's own
    kernels 2 to 5 times further than on the CPU (eval mode: the same as on the CPU)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield torch.device("cpu")
    finally:
        torch.set_num_threads(n)


def to_device(obj, dev):
    if isinstance(obj, torch.Tensor):
        return obj.to(dev)
    if isinstance(obj, dict):
        return {k: to_device(v, dev) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_device(v, dev) for v in obj)
    return obj


# --------------------------------------------------------------------------------------------------------------- state ----
def cast_state(state, dtype, device):
    """a private copy: floating tensors in `dtype` (parameters require a gradient), counters as they are"""
    out = {}
    for k, v in state.items():
        v = torch.as_tensor(v).detach().to(device)
        out[k] = v.to(dtype).clone().requires_grad_(M.is_param(k)) if v.is_floating_point() else v.clone()
    return out


def _buffers(st, training, strip=""):
    out = {}
    for k, v in st.items():
        if M.is_param(k):
            continue
        v = v.detach().clone()
        if k.endswith("num_batches_tracked") and training:
            v += 1
        out["b:" + k[len(strip):]] = v
    return out


def zero_keys(names, training, masked=False):
    """The gradients that are exactly zero in exact arithmetic: weight_encoding.3.bias always (the softmax is invariant under
    a shift of its logits); in training mode also every bias that a BatchNorm's mean subtraction removes -- the bias of a
    Linear straight in front of a BatchNorm (`X.0.bias` with `X.1.norm`), and linear_v.bias / linear_p_bias.3.bias, which
    reach only weight_encoding.1 and, as the same shift of every row, norm2.  masked: the neighbour table has -1 placeholders;
    the masked softmax weights of such a row no longer sum to 1, the shift differs from row to row and norm2 does not remove
    it.  -> {"g:" + bias name: "g:" + the same layer's weight name}"""
    names = set(names)
    out = {}
    for k in names:
        if not k.endswith(".bias") or ".norm." in k:
            continue
        stem = k[: -len(".bias")]
        always = stem.endswith("weight_encoding.3")
        in_front = stem.endswith(".0") and (stem[:-2] + ".1.norm.weight") in names
        attn = not masked and stem.endswith(("attn.linear_v", "attn.linear_p_bias.3"))
        if always or (training and (in_front or attn)):
            out["g:" + k] = "g:" + stem + ".weight"
    return out


# ----------------------------------------------------------------------------------------------------------- the block ----
def run_block(state, x, coord, idx, groups, go, training, keep=None, dtype=torch.float64, block=M._block, grads=True):
    """oracle.ptv2_ref._block under the prefix "blk" -> ({out, g_x, g:<parameter>, b:<buffer>}, Recorder); keep: the (n,)
    DropPath factor of the rows (training mode)"""
    dev = x.device
    st = cast_state({"blk." + k: v for k, v in state.items()}, dtype, dev)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    masks = {"blk": keep.to(dtype).view(-1, 1)} if keep is not None else None
    cx = M.Ctx(st, training, masks, update_stats=True)
    rec = Recorder()
    with recording(rec), torch.set_grad_enabled(grads), _own_batch_norm():
        out = block(cx, "blk", xx, coord.to(dtype), idx, groups)
    res = {"out": out.detach()}
    if grads:
        names = [k for k in st if M.is_param(k)]
        gs = torch.autograd.grad(out, [xx] + [st[k] for k in names], go.to(dtype))
        res["g_x"] = gs[0]
        res.update({"g:" + k[4:]: g for k, g in zip(names, gs[1:])})
    res.update(_buffers(st, training, strip="blk."))
    return res, rec


# ----------------------------------------------------------------------------------------------------------- the model ----
def oracle_tables(cfg, coord, offset):
    """The tables of a scene as the oracle builds them on the CPU (the GPU tests take them from model.geometry instead):
    per level dict(coord, knn {k: idx}, cluster, order, idx_ptr, up_idx, up_weight)."""
    from oracle import pointops_ref as P

    ns = len(cfg["enc_depths"])
    ks = [{cfg["patch_embed_neighbours"], cfg["dec_neighbours"][0]}]
    for i in range(ns):
        ks.append({cfg["enc_neighbours"][i]} | ({cfg["dec_neighbours"][i + 1]} if i + 1 < ns else set()))
    levels, c, o = [], coord, offset.long()
    for i in range(ns + 1):
        lv = dict(coord=c, knn={k: P.knn_query(k, c, o.int())[0] for k in sorted(ks[i])})
        if i < ns:
            nc, noff, cluster, order, idx_ptr = M.grid_pool_geometry(c, o, cfg["grid_sizes"][i])
            lv.update(cluster=cluster, order=order, idx_ptr=idx_ptr)
            if cfg["unpool_backend"] == "interp":
                lv["up_idx"], lv["up_weight"] = P.interpolation_weights(nc, c, noff.int(), o.int())
            c, o = nc, noff
        levels.append(lv)
    return levels


def forward_tables(cx, cfg, feat, levels, rec=None, mutate=()):
    """The statement sequence of oracle.ptv2_ref.forward (:556-576) on given tables.  mutate (host test): "drop_skip" leaves the
    decoder's contribution out of the gradient of the level-0 skip tensor; "pool_second" sends the gradient of one pooled
    value to the runner-up row.  Neither changes a forward value."""
    s = cx.s
    ns = len(cfg["enc_depths"])

    def relu(t):
        return M.F.relu(t)

    def seq(pre, depth, level, x, groups, k):
        lv = levels[level]
        for i in range(depth):
            x = M._block(cx, "%s.blocks.%d" % (pre, i), x, lv["coord"].to(x.dtype), lv["knn"][k], groups)
        return x

    x = relu(M._pbn(cx, TF.linear(feat, s["patch_embed.proj.0.weight"]), "patch_embed.proj.1"))
    x = seq("patch_embed.blocks", cfg["patch_embed_depth"], 0, x, cfg["patch_embed_groups"], cfg["patch_embed_neighbours"])
    skips = [x]
    for i in range(ns):
        pre, lv = "enc_stages.%d" % i, levels[i]
        d = relu(M._pbn(cx, TF.linear(x, s[pre + ".down.fc.weight"]), pre + ".down.norm"))
        order = lv["order"].long()
        if rec is not None:
            rec.pool(d, order, lv["idx_ptr"])
        x = M.segment_csr(d[order], lv["idx_ptr"], "max")
        if "pool_second" in mutate and i == 0:
            p = rec.pools[-1]
            at = torch.nonzero(torch.isfinite(p["gap"]) & (x.detach() > 0))[0]
            t = d[p["second"][at[0], at[1]], at[1]] - d[p["first"][at[0], at[1]], at[1]]
            bump = torch.zeros_like(x)
            bump[at[0], at[1]] = 1.0
            x = x + bump * (t - t.detach())
        x = seq(pre + ".blocks", cfg["enc_depths"][i], i + 1, x, cfg["enc_groups"][i], cfg["enc_neighbours"][i])
        skips.append(x)
    x = skips.pop()
    for i in reversed(range(ns)):
        pre, lv = "dec_stages.%d.up" % i, levels[i]
        skip = skips.pop()
        if "drop_skip" in mutate and i == 0:
            skip = skip.detach()
        proj = relu(M._pbn(cx, M._linear(cx, x, pre + ".proj.0"), pre + ".proj.1"))
        if cfg["unpool_backend"] == "map":
            up = proj[lv["cluster"]]
        else:
            idx, w = lv["up_idx"], lv["up_weight"].to(proj.dtype)
            up = torch.zeros(idx.shape[0], proj.shape[1], dtype=proj.dtype, device=proj.device)
            for j in range(idx.shape[1]):
                up = up + proj[idx[:, j].long(), :] * w[:, j].unsqueeze(-1)
        x = up + relu(M._pbn(cx, M._linear(cx, skip, pre + ".proj_skip.0"), pre + ".proj_skip.1"))
        x = seq("dec_stages.%d.blocks" % i, cfg["dec_depths"][i], i, x, cfg["dec_groups"][i], cfg["dec_neighbours"][i])
    if cfg["num_classes"] > 0:
        x = relu(M._pbn(cx, M._linear(cx, x, "seg_head.0"), "seg_head.1"))
        x = M._linear(cx, x, "seg_head.3")
    return x


def run_model(state, cfg, feat, levels, segment, training, dtype=torch.float64, grads=True, mutate=()):
    """-> ({logits, loss, g:<parameter>, b:<buffer>}, Recorder); loss = cross_entropy(logits, segment, ignore_index=-1)"""
    st = cast_state(state, dtype, feat.device)
    cx = M.Ctx(st, training, None, update_stats=True)
    rec = Recorder()
    with recording(rec), torch.set_grad_enabled(grads), _own_batch_norm():
        logits = forward_tables(cx, cfg, feat.to(dtype), levels, rec, mutate)
        loss = TF.cross_entropy(logits, segment, ignore_index=-1)
    res = {"logits": logits.detach(), "loss": loss.detach()}
    if grads:
        names = [k for k in st if M.is_param(k)]
        res.update({"g:" + k: g for k, g in zip(names, torch.autograd.grad(loss, [st[k] for k in names]))})
    res.update(_buffers(st, training))
    return res, rec


# ---------------------------------------------------------------------------------------------------------- the bound ----
def kind_of(key):
    return key if key in ("out", "logits", "loss", "g_x") else "buffer" if key.startswith("b:") else "grad"


def compare(Mk, got, f64, f32, zeros, tag, peaks=("out", "logits"), keys=None):
    """The M-rule in its absolute form, |ours - f64| <= M[kind] * max(|eager fp32 - f64|, 2^-24 |f64|), in L2 and for `peaks`
    also in the largest element; num_batches_tracked exactly; a zero key (zero_keys) must be zero in float64 to 1e-9 of its
    layer's weight gradient and is held to M["zero"] * max(|eager fp32|, 2^-24 |f64 weight gradient|).  Prints one
    ptv2-f64-ratio line per figure and returns the list of misses."""
    keys = sorted(f64) if keys is None else keys
    assert set(keys) <= set(got) and set(keys) <= set(f32), (set(keys) - set(got), set(keys) - set(f32))
    bad = []

    def line(kind, name, err, base):
        ratio = err / base if base > 0 else (0.0 if err == 0 else float("inf"))
        print("ptv2-f64-ratio %-28s %-6s %-58s err %.3e base %.3e ratio %.3f" % (tag, kind, name, err, base, ratio))
        if not err <= Mk[kind] * base:
            bad.append((name, err, Mk[kind] * base))

    for key in keys:
        g, r64, r32 = got[key], f64[key], f32[key]
        assert tuple(g.shape) == tuple(r64.shape), key
        if key.endswith("num_batches_tracked"):
            if int(g) != int(r64):
                bad.append((key, int(g), int(r64)))
            continue
        assert bool(torch.isfinite(g).all()), key
        g, r32 = g.double(), r32.double()
        if key in zeros:
            wnorm = float(f64[zeros[key]].norm())
            assert float(r64.norm()) <= 1e-9 * wnorm, (key, float(r64.norm()), wnorm)
            line("zero", key, float(g.norm()), max(float(r32.norm()), FLOOR * wnorm))
            continue
        kind = kind_of(key)
        line(kind, key, float((g - r64).norm()), max(float((r32 - r64).norm()), FLOOR * float(r64.norm())))
        if key in peaks:
            line(kind, key + " (peak)", float((g - r64).abs().max()),
                 max(float((r32 - r64).abs().max()), FLOOR * float(r64.abs().max())))
    return bad
