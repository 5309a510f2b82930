"""tests/golden/make_golden_msc.py -- the MSC-v1m1 fixtures, produced by CONSTRUCTING and RUNNING the reference's model on the CPU:

    msc_manifest.json   keys and shapes of MaskedSceneContrast over the default SpUNet-v1m1 backbone, with both reconstruction
                        heads and with none
    msc_configs.json    the `model` dict and the training transform lists of the reference's two MSC-v1m1 ScanNet configs,
                        read by running the config files: settings only, what tests and tools/bench_msc.py build from
    msc.npz             one batch of two scenes (a few hundred points per view): the inputs, the recorded backbone outputs, the
                        state, the random tensors the reference drew (torch.randperm / torch.randint are wrapped), both masks,
                        match_index and every entry of the returned dict, for
                          a.*  color + normal heads, mask_rate 0.4, nce_t 0.4, matching_max_pair below the number of matches
                          b.*  no heads, mask_rate 0, nce_t 0.07
                        and a numpy run of the reference's RandomColorJitter (cj.*): each adjustment alone with its factor, and
                        one whole call with its draws

The reference's masked_scene_contrast_v1m1_base.py is imported by path under the stub packages of make_golden_spunet.py,
its own pointcept/models/utils.py, `torch_geometric.nn.pool.voxel_grid` = oracle/ptv2_ref.py::voxel_grid, torch's trunc_normal_,
a `pointops.knn_query` that calls tests/msc_ref.py::knn_bruteforce, a `build_model` that looks the class up, and
torch.Tensor.cuda made the identity (:106 calls it).  The backbone is replaced by a module that returns recorded features.
Only data is written.  Every kNN distance stays a relative MARGIN away from the matching radius.

usage:  python tests/golden/make_golden_msc.py <reference root>
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
sys.path.insert(0, HERE)

import make_golden_spunet as MS  # noqa: E402
from oracle import ptv2_ref  # noqa: E402
from tests import msc_ref as R  # noqa: E402

SEED = 70
MARGIN = 1e-4   # relative distance of every kNN distance from RADIUS
RADIUS = 0.1
MAX_K = 8
WIDTH = 16      # channels of the recorded backbone output
BASE = 380      # points of a scene before the views are taken


class Recorded(nn.Module):
    """returns the recorded features of view 1, then of view 2"""

    def __init__(self, feats):
        super().__init__()
        self.feats, self.calls = feats, 0

    def forward(self, data_dict):
        self.calls += 1
        return self.feats[(self.calls - 1) % 2]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def load_reference(ref):
    models = MS.load_reference(ref)
    builder = sys.modules["pointcept.models.builder"]
    builder.build_model = lambda cfg: cfg if isinstance(cfg, nn.Module) else models[cfg["type"]](**{k: v for k, v in cfg.items() if k != "type"})
    for name, attrs in (("torch_geometric.nn", {}), ("torch_geometric.nn.pool", {"voxel_grid": ptv2_ref.voxel_grid}),
                        ("pointcept.utils", {}), ("pointcept.utils.comm", {"get_world_size": lambda: 1})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    pointops = types.ModuleType("pointops")

    def knn_query(nsample, xyz, offset, new_xyz, new_offset):
        idx, d2 = R.knn_bruteforce(nsample, xyz.numpy(), offset.numpy(), new_xyz.numpy(), new_offset.numpy())
        return torch.from_numpy(idx), torch.sqrt(torch.from_numpy(d2))

    pointops.knn_query = knn_query
    sys.modules["pointops"] = pointops
    _load("pointcept.models.utils", os.path.join(ref, "pointcept", "models", "utils.py"))
    folder = os.path.join(ref, "pointcept", "models", "masked_scene_contrast")
    pkg = types.ModuleType("pointcept.models.masked_scene_contrast")
    pkg.__path__ = [folder]
    sys.modules["pointcept.models.masked_scene_contrast"] = pkg
    _load("pointcept.models.masked_scene_contrast.masked_scene_contrast_v1m1_base",
          os.path.join(folder, "masked_scene_contrast_v1m1_base.py"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    return models


def load_transforms(ref):
    """the reference's datasets/transform.py under a registry that only files the classes"""
    class Registry:
        def __init__(self, name):
            self.name = name

        def register_module(self, *a, **k):
            return lambda cls: cls

    registry = types.ModuleType("pointcept.utils.registry")
    registry.Registry = Registry
    sys.modules["pointcept.utils.registry"] = registry
    pkg = types.ModuleType("pointcept.datasets")
    pkg.__path__ = []
    sys.modules["pointcept.datasets"] = pkg
    return _load("pointcept.datasets.transform", os.path.join(ref, "pointcept", "datasets", "transform.py"))


def make_batch(seed):
    """two centred scenes; view 1 and view 2 are subsets of the same points, view 2 moved by less than 4 mm per axis"""
    rng = np.random.default_rng(seed)
    out = {}
    for view in (1, 2):
        out[view] = dict(origin=[], color=[], normal=[], out=[])
    for scene, extent in enumerate(((1.2, 1.0, 0.5), (0.7, 1.6, 0.4))):
        n = BASE - 60 * scene
        base = (rng.uniform(0.0, 1.0, (n, 3)) * np.array(extent) - np.array([extent[0] / 2, extent[1] / 2, 0.0])).astype(np.float32)
        color = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        normal = rng.normal(0.0, 1.0, (n, 3))
        normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
        feature = rng.normal(0.3, 1.0, (n, WIDTH))  # what a backbone would say of a point: matched rows are similar
        for view in (1, 2):
            keep = np.sort(rng.permutation(n)[:int(n * 0.75)])
            moved = base[keep] + (rng.uniform(-0.004, 0.004, (len(keep), 3)).astype(np.float32) if view == 2 else np.float32(0))
            out[view]["origin"].append(moved.astype(np.float32))
            out[view]["color"].append(color[keep])
            out[view]["normal"].append(normal[keep])
            out[view]["out"].append((feature[keep] + rng.normal(0.0, 0.4, (len(keep), WIDTH))).astype(np.float32))
    batch = {}
    for view in (1, 2):
        v = out[view]
        origin = np.concatenate(v["origin"])
        batch["view%d_origin_coord" % view] = origin
        batch["view%d_coord" % view] = (origin * np.float32(1.05) + np.float32(0.01 * view)).astype(np.float32)
        batch["view%d_color" % view] = np.concatenate(v["color"])
        batch["view%d_normal" % view] = np.concatenate(v["normal"])
        batch["view%d_feat" % view] = np.concatenate([batch["view%d_color" % view], batch["view%d_normal" % view]], 1)
        batch["view%d_offset" % view] = np.cumsum([len(o) for o in v["origin"]]).astype(np.int32)
        batch["view%d_out" % view] = np.concatenate(v["out"])
    return batch


def margin_of(batch):
    idx, d2 = R.knn_bruteforce(MAX_K, batch["view2_origin_coord"], batch["view2_offset"], batch["view1_origin_coord"], batch["view1_offset"])
    d = np.sqrt(d2[idx >= 0].astype(np.float64))
    return np.abs(d - RADIUS).min() / RADIUS, int((R.hit_counts(idx, d2, RADIUS) > 0).sum())


def record_model(cls, batch, out, prefix, seed, **cfg):
    drawn = []
    randperm, randint = torch.randperm, torch.randint

    def rec(kind, fn):
        def wrapped(*a, **k):
            value = fn(*a, **k)
            drawn.append((kind, value.clone()))
            return value
        return wrapped

    torch.manual_seed(seed)
    backbone = Recorded([torch.from_numpy(batch["view1_out"]), torch.from_numpy(batch["view2_out"])])
    model = cls(backbone=backbone, backbone_in_channels=6, backbone_out_channels=WIDTH, matching_max_k=MAX_K, matching_max_radius=RADIUS,
                **cfg).train()
    with torch.no_grad():
        for head in (model.color_head, model.normal_head):
            if head is not None:
                head.weight.normal_(0.0, 0.3)
                head.bias.normal_(0.0, 0.1)
    masks, pairs = [], []
    gen, match = model.generate_cross_masks, model.match_contrastive_pair
    model.generate_cross_masks = lambda *a, **k: masks.append(gen(*a, **k)) or masks[-1]
    model.match_contrastive_pair = lambda *a, **k: pairs.append(match(*a, **k)) or pairs[-1]
    torch.randperm, torch.randint = rec("randperm", randperm), rec("randint", randint)
    try:
        with torch.no_grad():
            res = model({k: torch.from_numpy(v) for k, v in batch.items() if not k.endswith("_out")})
    finally:
        torch.randperm, torch.randint = randperm, randint
    kinds = [k for k, _ in drawn]
    assert kinds[:2] == ["randperm", "randint"] and kinds[2:] in ([], ["randperm"]), kinds
    out[prefix + "mask_perm"] = drawn[0][1].numpy()
    out[prefix + "match_draws"] = drawn[1][1].numpy()
    out[prefix + "pair_perm"] = drawn[2][1].numpy() if len(drawn) > 2 else np.zeros(0, np.int64)
    out[prefix + "mask1"], out[prefix + "mask2"] = (m.numpy() for m in masks[0])
    out[prefix + "match_index"] = pairs[0].numpy()
    for k, v in model.state_dict().items():
        if not k.startswith("backbone."):
            out[prefix + "state." + k] = v.numpy()
    for k, v in res.items():
        out[prefix + "result." + k] = np.asarray(v.numpy())
    return res


def record_color_jitter(T, out, seed):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 255.0, (300, 3)).astype(np.float32)
    color[:8] = np.array([[0, 0, 0], [255, 255, 255], [17, 17, 17], [255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 200, 200], [200, 9, 200]], np.float32)
    jitter = T.RandomColorJitter(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.02, p=0.8)
    out["cj.color"] = color
    for name, factor in (("brightness", 1.23), ("brightness", 0.71), ("contrast", 1.31), ("contrast", 0.64), ("saturation", 1.17),
                         ("saturation", 0.83), ("hue", 0.0173), ("hue", -0.0191), ("hue", 0.5)):
        got = getattr(jitter, "adjust_" + name)(color.copy(), factor)
        assert got.dtype == np.float32
        out["cj.%s.%r" % (name, factor)] = got
    # one whole call: the draws in the order the reference takes them
    uniform, rand, randperm = np.random.uniform, np.random.rand, torch.randperm
    drawn = dict(order=None, factors=[], gates=[])
    np.random.seed(seed)
    torch.manual_seed(seed)
    np.random.uniform = lambda lo, hi: drawn["factors"].append(uniform(lo, hi)) or drawn["factors"][-1]
    np.random.rand = lambda: drawn["gates"].append(rand()) or drawn["gates"][-1]

    def perm(n):
        drawn["order"] = randperm(n)
        return drawn["order"]

    torch.randperm = perm
    try:
        full = jitter(dict(color=color.copy()))["color"]
    finally:
        np.random.uniform, np.random.rand, torch.randperm = uniform, rand, randperm
    assert len(drawn["factors"]) == 4 and len(drawn["gates"]) == 4
    out["cj.full"] = full
    out["cj.full.order"] = drawn["order"].numpy()
    out["cj.full.factors"] = np.asarray(drawn["factors"], np.float64)
    out["cj.full.gates"] = np.asarray(drawn["gates"], np.float64)  # by position in order: every adjustment is switched on


def record_configs(ref):
    import runpy

    out = {}
    for name, file in (("base", "pretrain-msc-v1m1-0-spunet-base.py"), ("pointcontrast", "pretrain-msc-v1m1-1-spunet-pointcontrast.py")):
        cfg = runpy.run_path(os.path.join(ref, "configs", "scannet", file))
        out[name] = dict(config="configs/scannet/" + file, model=cfg["model"],
                         **{k: v for k, v in cfg["data"]["train"].items() if k.endswith("transform")})
    path = os.path.join(HERE, "msc_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("msc_configs.json", os.path.getsize(path), "bytes,", {k: sorted(v) for k, v in out.items()})


def main():
    ref = sys.argv[1]
    record_configs(ref)
    models = load_reference(ref)
    cls = models["MSC-v1m1"]
    backbone = dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                    layers=(2, 3, 4, 6, 2, 2, 2, 2))
    manifest = {}
    for name, heads in (("heads", True), ("no_heads", False)):
        model = cls(backbone=dict(backbone), backbone_in_channels=6, backbone_out_channels=96, reconstruct_color=heads,
                    reconstruct_normal=heads)
        manifest[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
    path = os.path.join(HERE, "msc_manifest.json")
    with open(path, "w") as f:  # compact, one key per line
        f.write("{\n%s\n}\n" % ",\n".join(' %s: {\n%s\n }' % (json.dumps(name), ",\n".join(
            "  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in keys.items())) for name, keys in manifest.items()))
    print("msc_manifest.json", os.path.getsize(path), "bytes,", {k: len(v) for k, v in manifest.items()}, "keys")

    for seed in range(SEED, SEED + 100):  # the first seed whose distances keep the margin
        batch = make_batch(seed)
        margin, matched = margin_of(batch)
        if margin > MARGIN:
            break
    assert margin > MARGIN, "no seed keeps the margin"
    out = dict(batch, seed=np.array(seed, np.int64), radius=np.array(RADIUS), max_k=np.array(MAX_K, np.int64))
    a = record_model(cls, batch, out, "a.", seed + 1, mask_grid_size=0.1, mask_rate=0.4, nce_t=0.4, matching_max_pair=matched - 100,
                     reconstruct_color=True, reconstruct_normal=True)
    b = record_model(cls, batch, out, "b.", seed + 2, mask_grid_size=0.1, mask_rate=0, nce_t=0.07, matching_max_pair=8192,
                     reconstruct_color=False, reconstruct_normal=False)
    out["a.max_pair"] = np.array(matched - 100, np.int64)
    assert len(out["a.match_index"]) == matched - 100 and len(out["a.pair_perm"]) == matched and len(out["b.match_index"]) == matched
    assert out["a.mask1"].any() and out["a.mask2"].any() and not out["b.mask1"].any() and not out["b.mask2"].any()
    record_color_jitter(load_transforms(ref), out, seed + 3)
    path = os.path.join(HERE, "msc.npz")
    np.savez_compressed(path, **out)
    print("msc.npz", os.path.getsize(path), "bytes, seed", seed, ", margin %.2e," % margin, matched, "matched rows,",
          {k: float(v) for k, v in a.items()}, {k: float(v) for k, v in b.items()})


if __name__ == "__main__":
    main()
