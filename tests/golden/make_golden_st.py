"""tests/golden/make_golden_st.py -- the Stratified Transformer fixtures, produced by EXECUTING the reference's
stratified_transformer_v1m2_refine.py on the CPU:

    st_manifest.json     keys and shapes of ST-v1m2 with the reference's default arguments and with tests/st_cases.MODEL_CONFIG
    st_model_st2.npz, st_model_st3.npz
                         the small configuration (train mode) on the two- and three-cloud batch of tests/st_cases.py: the pair
                         sets of every block as sorted (query, key) rows; float64 logits, loss and the gradient of every parameter
                         of at most 4096 elements; the fp32 logits and loss; the fp32 run's own distance from float64
                         (dist/: relative L2, adist/: absolute L2, peak/: largest element over the largest reference element); the same for the
                         eval-mode logits

The reference's file is imported by path under stub packages: `pointops2.pointops` (farthest point sampling and kNN from the
oracle, the three attention operators from tests/st_ref.py), `torch_scatter`, `timm`, `torch_geometric.nn.pool`,
`torch_points_kernels` and the two `torch_points3d` modules from tests/st_ref.py; `.cuda()` and `torch.cuda.IntTensor` are mapped
to the CPU.  Coordinates stay fp32 in the float64 run: the cells and the relative-position index are integer quantities of the
fp32 coordinates, and the stubs raise them to float64 where the mathematics is continuous; the reference's own `.float()`
casts are switched off in that run.  Nothing of the reference is copied:
only arrays are written.  Weights come from tests/st_cases.fill_state.

usage:  python tests/golden/make_golden_st.py <reference root>            writes the files
        python tests/golden/make_golden_st.py <reference root> --seeds    prints the first usable seed of each batch
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pointops_ref as P  # noqa: E402
from tests import st_cases as SC  # noqa: E402
from tests import st_ref as R  # noqa: E402

RECORD = []   # (index_0, index_1, coords, window_size, quant_size) of every attention call of one forward


def _index_0(offsets, m):
    counts = (offsets[1:] - offsets[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.numel()), counts, output_size=m)


def _pointops2():
    stub = types.ModuleType("pointops2.pointops")

    def furthestsampling(xyz, offset, new_offset):
        return P.farthest_point_sampling(xyz.float(), offset.int(), new_offset.int())

    def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
        assert idx is None and not use_xyz
        idx = P.knn_query_raw(nsample, xyz.float(), offset.int(), new_xyz.float(), new_offset.int(), pad_with_start=True)[0]
        return feat[idx.long()]

    def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
        idx = P.knn_query_raw(k, xyz.float(), offset.int(), new_xyz.float(), new_offset.int())[0].long()
        dist = (new_xyz.to(feat.dtype).unsqueeze(1) - xyz.to(feat.dtype)[idx]).pow(2).sum(-1).sqrt()
        dist_recip = 1.0 / (dist + 1e-8)
        weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
        return (feat[idx] * weight.unsqueeze(-1)).sum(1)

    def attention_step1_v2(q, k, index1, index0_offsets, n_max):
        return R.attention_step1(q, k, _index_0(index0_offsets, index1.numel()), index1.long())

    def dot_prod_with_idx_v3(q, index_q_offsets, n_max, k, index_k, table_q, table_k, rel_idx):
        return R.dot_prod_with_idx(q, k, _index_0(index_q_offsets, index_k.numel()), index_k.long(), table_q, table_k, rel_idx.long())

    def attention_step2_with_rel_pos_value_v2(attn, v, index0_offsets, n_max, index1, table, rel_idx):
        return R.attention_step2(attn, v, _index_0(index0_offsets, index1.numel()), index1.long(), table, rel_idx.long())

    for fn in (furthestsampling, queryandgroup, interpolation, attention_step1_v2, dot_prod_with_idx_v3,
               attention_step2_with_rel_pos_value_v2):
        setattr(stub, fn.__name__, fn)
    return stub


class _KPConvLayer(nn.Module):
    def __init__(self, num_inputs, num_outputs, point_influence, add_one=False):
        super().__init__()
        assert not add_one
        self.KP_extent = point_influence
        self.K_points = nn.Parameter(R.kernel_points(point_influence), requires_grad=False)
        self.weight = nn.Parameter(torch.empty(15, num_inputs, num_outputs))
        nn.init.xavier_normal_(self.weight)

    def forward(self, query_points, support_points, neighbors, x):
        return R.kpconv(support_points.to(x.dtype), neighbors, x, self.weight, self.K_points.to(x.dtype), self.KP_extent)


class _FastBatchNorm1d(nn.Module):
    def __init__(self, num_features, momentum=0.1):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(num_features, momentum=momentum)

    def forward(self, x):
        return self.batch_norm(x)


class _DropPath(nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        assert self.drop_prob == 0.0 or not self.training   # (the fixtures run with drop_path_rate = 0)
        return x


def load_reference(ref):
    models = {}

    class Registry:
        def register_module(self, name=None, **_):
            def deco(cls):
                models[name] = cls
                return cls
            return deco

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    p2 = _pointops2()
    module("pointops2", pointops=p2)
    sys.modules["pointops2.pointops"] = p2
    module("torch_scatter", scatter_softmax=lambda src, index, dim=0: R.scatter_softmax(src, index, int(index.max()) + 1))
    module("timm")
    module("timm.models")
    module("timm.models.layers", DropPath=_DropPath, trunc_normal_=torch.nn.init.trunc_normal_)
    module("torch_geometric")
    module("torch_geometric.nn")
    module("torch_geometric.nn.pool", voxel_grid=lambda pos, batch, size, start=None: R.cluster_ids(
        R.voxel_cells(pos, size, pos.float().min(0).values if start is None else start), batch))
    module("torch_points_kernels", ball_query=lambda r, max_n, x, y, mode=None, batch_x=None, batch_y=None: (
        R.ball_query(r, max_n, x, batch_x), None))
    module("torch_points3d")
    module("torch_points3d.modules")
    module("torch_points3d.modules.KPConv")
    module("torch_points3d.modules.KPConv.kernels", KPConvLayer=_KPConvLayer)
    module("torch_points3d.core")
    module("torch_points3d.core.common_modules", FastBatchNorm1d=_FastBatchNorm1d)
    module("pointcept")
    module("pointcept.models")
    module("pointcept.models.builder", MODELS=Registry())
    torch.cuda.IntTensor = torch.IntTensor
    torch.Tensor.cuda = lambda self, *a, **k: self
    name = "pointcept.models.stratified_transformer_v1m2_refine"
    path = os.path.join(ref, "pointcept", "models", "stratified_transformer", "stratified_transformer_v1m2_refine.py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    # record the pairs every attention call receives
    inner = mod.WindowAttention.forward

    def recording(self, feats, coords, index_0, index_1, index_0_offsets, n_max):
        RECORD.append((index_0.clone(), index_1.clone(), coords.clone(), self.window_size, self.quant_size))
        return inner(self, feats, coords, index_0, index_1, index_0_offsets, n_max)

    mod.WindowAttention.forward = recording

    # Block.forward :262-269 ends in `feats += self.drop_path(self.mlp(self.norm2(feats)))`, an in-place add to the tensor norm2
    # has saved for its backward, which autograd refuses on the CPU.  The same statements with the sum written out of place:
    def block_forward(self, feats, coords, index_0, index_1, index_0_offsets, n_max):
        short_cut = feats
        feats = self.norm1(feats)
        feats = self.attn(feats, coords, index_0, index_1, index_0_offsets, n_max)
        feats = short_cut + self.drop_path(feats)
        return feats + self.drop_path(self.mlp(self.norm2(feats)))

    mod.Block.forward = block_forward
    return mod, models


def make_model(models, dtype):
    model = models["ST-v1m2"](**SC.MODEL_CONFIG)
    state = SC.fill_state({k: tuple(v.shape) for k, v in model.state_dict().items()})
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith(("K_points", "num_batches_tracked")) for k in missing.missing_keys)
    return model.to(dtype)


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def peak(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def step(models, batch, dtype, train):
    """In the float64 run the reference's `.float()` casts in front of the attention operators are switched off: every tensor
    they meet is either continuous (and float64 on purpose) or a function of the coordinates, which are fp32 already."""
    keep = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self
    try:
        return _step(models, batch, dtype, train)
    finally:
        torch.Tensor.float = keep


def _step(models, batch, dtype, train):
    del RECORD[:]
    model = make_model(models, dtype).train(train)
    data = dict(coord=batch["coord"], feat=batch["feat"].to(dtype), offset=batch["offset"])
    if not train:
        with torch.no_grad():
            return {"eval_logits": model(data)}
    logits = model(data)
    loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
    loss.backward()
    res = {"logits": logits.detach(), "loss": loss.detach()}
    for key, p in model.named_parameters():
        if p.grad is not None and p.numel() <= SC.SMALL_PARAMETER:
            res["g:" + key] = p.grad
    return res


def device_rel_index(coords, index_0, index_1, window_size, quant_size):
    """:145-151 as the GPU evaluates them: a division by a python scalar multiplies by the scalar's fp32 reciprocal"""
    c = coords.float().numpy()
    rp = c[index_0.numpy()] - c[index_1.numpy()]
    rp = np.rint(rp * np.float32(100000)) * (np.float32(1) / np.float32(100000))
    t = ((rp + np.float32(2 * window_size)) - np.float32(1e-4)) * (np.float32(1) / np.float32(quant_size))
    return np.trunc(t).astype(np.int64)


def usable(models, name, seed):
    batch = {k: torch.from_numpy(v) for k, v in SC.model_batch(name, seed).items()}
    try:
        step(models, batch, torch.float32, False)
    except AssertionError:
        return False
    for index_0, index_1, coords, w, q in RECORD:
        want, ok = R.rel_index(coords, index_0, index_1, w, q)
        if not ok or not np.array_equal(device_rel_index(coords, index_0, index_1, w, q), want.numpy()):
            return False
    return True


def fixture(models, name):
    batch = {k: torch.from_numpy(v) for k, v in SC.model_batch(name).items()}
    out, runs = {}, {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        runs[tag] = step(models, batch, dtype, True)
        pairs = [torch.stack([a, b], 1) for a, b, _, _, _ in RECORD]
        if tag == "f64":
            for i, p in enumerate(pairs):
                out["pairs/%d" % i] = p.numpy().astype(np.int32)
        else:  # the integer quantities of both runs are the same function of the same fp32 coordinates
            assert all(np.array_equal(out["pairs/%d" % i], p.numpy()) for i, p in enumerate(pairs))
        runs[tag].update(step(models, batch, dtype, False))
    for key, v in runs["f64"].items():
        out["f64/" + key] = v.numpy()
        if not key.startswith("g:"):
            out["f32/" + key] = runs["f32"][key].numpy()
        out["dist/" + key] = np.float64(rel_l2(runs["f32"][key], v))
        out["adist/" + key] = np.float64((runs["f32"][key].double() - v).norm())
    for key in ("logits", "eval_logits"):
        out["peak/" + key] = np.float64(peak(runs["f32"][key], runs["f64"][key]))
    return out


def main():
    P.build()
    torch.use_deterministic_algorithms(True)   # index_add_ in index order: two runs of the reference give the same bits
    mod, models = load_reference(sys.argv[1])
    assert models["ST-v1m2"] is models["STv1m2"] if "STv1m2" in models else True
    if sys.argv[2:] == ["--seeds"]:
        for name in SC.MODEL_CLOUDS:
            print(name, "seed", next(s for s in range(1000) if usable(models, name, s)))
        return
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}  # noqa: E731
    manifest = {"default": shapes(models["ST-v1m2"](in_channels=6, num_classes=20)),
                "small": shapes(models["ST-v1m2"](**SC.MODEL_CONFIG))}
    with open(os.path.join(HERE, "st_manifest.json"), "w") as f:
        text = [" %s: {\n%s\n }" % (json.dumps(name), ",\n".join(
            "  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in keys.items()))
            for name, keys in manifest.items()]
        f.write("{\n%s\n}\n" % ",\n".join(text))
    for name in SC.MODEL_CLOUDS:
        assert usable(models, name, SC.MODEL_SEEDS[name]), "tests/st_cases.MODEL_SEEDS[%r] is not usable: run --seeds" % name
        np.savez_compressed(os.path.join(HERE, "st_model_%s.npz" % name), **fixture(models, name))
    for name in ["st_manifest.json"] + ["st_model_%s.npz" % n for n in SC.MODEL_CLOUDS]:
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
