"""tests/golden/make_golden_ptv1.py -- the Point Transformer V1 fixtures, produced by EXECUTING the reference's model on the CPU:

    ptv1_manifest.json   keys and shapes of PointTransformer-Seg26 / 38 / 50
    ptv1_layer.npz       the reference layer (fp32) on two cases of tests/ptv1_cases.py: out, input and parameter gradients
    ptv1_model.npz       Seg26 (train mode) on the two-cloud batch of tests/ptv1_cases.py: float64 logits, loss, gradient of
                         feat and buffers of a .double() copy, the fp32 results, and the fp32 run's own distance from
                         float64 (dist/: relative L2, adist/: absolute L2, peak/: largest element)
    ptv1_model_eval.npz  the same for the eval-mode logits
    ptv1_model_grads_enc.npz, ptv1_model_grads_dec.npz
                         the float64 gradient of every parameter of at most 4096 elements (encoder / decoder and head) and
                         the fp32 run's distance from it (several files: no committed file is larger than 1 MiB)

The reference's pointcept/models/point_transformer/point_transformer_seg.py and utils.py are imported by path under stub
packages: `pointops` is oracle/pointops_ref.py (knn_query, farthest_point_sampling, grouping, interpolation,
knn_query_and_group), `pointcept.models.builder.MODELS` a registry that only records, `torch.cuda.IntTensor` a CPU int32
tensor.  Nothing of the reference is copied: only arrays are written.  Weights are never stored: tests/ptv1_cases.fill_state
fills a state dict from a seed, here and in the tests.

usage:  python tests/golden/make_golden_ptv1.py <reference root>            writes the files
        python tests/golden/make_golden_ptv1.py --seeds                     prints, per layer case, the first seed whose
                                                                            float64 ReLU pre-activations keep ptv1_cases.MARGIN
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pointops_ref as P  # noqa: E402
from tests import ptv1_cases as PC  # noqa: E402
from tests import ptv1_ref as R  # noqa: E402

NAMES = ("PointTransformer-Seg26", "PointTransformer-Seg38", "PointTransformer-Seg50")
SMALL = 4096
BUFFERS_OF = ("enc1.1.transformer.linear_w.0", "enc5.1.bn2")


def load_reference(ref):
    """the reference's module, imported by path under stub packages"""
    models = {}

    class Registry:
        def register_module(self, name=None, **_):
            def deco(cls):
                models[name] = cls
                return cls
            return deco

    stub = types.ModuleType("pointops")
    for fn in ("knn_query", "farthest_point_sampling", "grouping", "interpolation", "knn_query_and_group"):
        setattr(stub, fn, getattr(P, fn))
    sys.modules["pointops"] = stub
    folder = os.path.join(ref, "pointcept", "models", "point_transformer")
    for name, path in (("pointcept", None), ("pointcept.models", None), ("pointcept.models.point_transformer", folder)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path] if path else []
        sys.modules[name] = pkg
    builder = types.ModuleType("pointcept.models.builder")
    builder.MODELS = Registry()
    sys.modules["pointcept.models.builder"] = builder
    torch.cuda.IntTensor = lambda values: torch.tensor(values, dtype=torch.int32)
    for leaf in ("utils", "point_transformer_seg"):
        name = "pointcept.models.point_transformer." + leaf
        spec = importlib.util.spec_from_file_location(name, os.path.join(folder, leaf + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules["pointcept.models.point_transformer.point_transformer_seg"], models


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def layer_fixture(module):
    out = {}
    for name in PC.GOLDEN_LAYER_CASES:
        c = PC.case(name)
        t = {k: torch.from_numpy(v) for k, v in PC.layer_inputs(c).items()}
        layer = module.PointTransformerLayer(c.c, c.c, 8, c.ns)
        layer.load_state_dict(PC.layer_state(layer, c), strict=True)
        layer.train()
        x = t["x_q"].clone().requires_grad_(True)
        offset = torch.tensor(np.cumsum(c.clouds), dtype=torch.int32)
        y = layer([t["coord"], x, offset])
        params = dict(layer.named_parameters())
        grads = torch.autograd.grad(y, [x] + list(params.values()), t["g_out"])
        out[name + "/out"] = y.detach().numpy()
        out[name + "/g_x"] = grads[0].numpy()
        for key, g in zip(params, grads[1:]):
            out[name + "/g:" + key] = g.numpy()
    return out


def model_step(model, batch, dtype):
    model = model.to(dtype).train()
    feat = batch["feat"].to(dtype).requires_grad_(True)
    logits = model(dict(coord=batch["coord"].to(dtype), feat=feat, offset=batch["offset"]))
    loss = torch.nn.functional.cross_entropy(logits, batch["segment"])
    loss.backward()
    res = {"logits": logits.detach(), "loss": loss.detach(), "g_feat": feat.grad}
    for key, p in model.named_parameters():
        if p.numel() <= SMALL:
            res["g:" + key] = p.grad
    state = model.state_dict()
    for stem in BUFFERS_OF:
        for leaf in ("running_mean", "running_var", "num_batches_tracked"):
            res["b:%s.%s" % (stem, leaf)] = state["%s.%s" % (stem, leaf)].clone()
    return res


def model_eval(model, batch, dtype):
    model = model.to(dtype).eval()
    with torch.no_grad():
        return model(dict(coord=batch["coord"].to(dtype), feat=batch["feat"].to(dtype), offset=batch["offset"]))


def model_fixture(models):
    batch = {k: torch.from_numpy(v) for k, v in PC.model_batch().items()}
    make = lambda: models["PointTransformer-Seg26"](in_channels=6, num_classes=13)  # noqa: E731
    state = PC.fill_state(PC.shapes_of(make()), PC.MODEL_SEED)
    runs = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        model = make()
        model.load_state_dict(state, strict=True)
        runs[tag + "eval"] = model_eval(model, batch, dtype)
        model = make()
        model.load_state_dict(state, strict=True)
        runs[tag] = model_step(model, batch, dtype)
    out = {}
    for key, v in runs["f64"].items():
        out["f64/" + key] = v.numpy()
        if key.endswith("num_batches_tracked"):
            continue
        if not key.startswith("g:"):  # (the fp32 parameter gradients are not kept: three files of at most 1 MiB)
            out["f32/" + key] = runs["f32"][key].numpy()
        out["dist/" + key] = np.float64(rel_l2(runs["f32"][key], v))
        out["adist/" + key] = np.float64((runs["f32"][key].double() - v).norm())
    out["peak/logits"] = np.float64((runs["f32"]["logits"].double() - runs["f64"]["logits"]).abs().max())
    out["f64/eval_logits"] = runs["f64eval"].numpy()
    out["f32/eval_logits"] = runs["f32eval"].numpy()
    out["dist/eval_logits"] = np.float64(rel_l2(runs["f32eval"], runs["f64eval"]))
    out["peak/eval_logits"] = np.float64((runs["f32eval"].double() - runs["f64eval"]).abs().max())
    return out


def find_seeds():
    for c in PC.LAYER_CASES:
        for seed in range(1000):
            t = {k: torch.from_numpy(v) for k, v in PC.layer_inputs(c, seed).items()}
            layer = R.Layer(c.c, c.ns)
            layer.load_state_dict(PC.layer_state(layer, c, seed))
            layer = layer.double().train()
            layer.attention(t["x_q"].double(), t["x_k"].double(), t["x_v"].double(), t["coord"].double(), t["idx"])
            if layer.margin() > PC.MARGIN:
                break
        print(c.name, "seed", seed, "margin %.3e" % layer.margin())


def main():
    if sys.argv[1:] == ["--seeds"]:
        return find_seeds()
    P.build()
    # torch's CPU index_put(accumulate=True), the backward of every gather here, adds with atomics from several threads: two runs
    # of the reference differ by 1e-6 in the gradient of feat.  The deterministic form adds in index order; the tests use it too
    torch.use_deterministic_algorithms(True)
    module, models = load_reference(sys.argv[1])
    manifest = {name: {k: list(v.shape) for k, v in models[name](in_channels=6, num_classes=13).state_dict().items()}
                for name in NAMES}
    with open(os.path.join(HERE, "ptv1_manifest.json"), "w") as f:  # compact, one key per line
        models_text = [" %s: {\n%s\n }" % (json.dumps(name), ",\n".join(
            "  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in keys.items()))
            for name, keys in manifest.items()]
        f.write("{\n%s\n}\n" % ",\n".join(models_text))
    np.savez_compressed(os.path.join(HERE, "ptv1_layer.npz"), **layer_fixture(module))
    fixture = model_fixture(models)
    part = lambda key: ("grads_enc" if "/g:enc" in key else "grads_dec") if "/g:" in key else "eval" if "eval" in key else "model"  # noqa: E731
    for which in ("model", "eval", "grads_enc", "grads_dec"):
        name = "ptv1_model.npz" if which == "model" else "ptv1_model_%s.npz" % which
        np.savez_compressed(os.path.join(HERE, name), **{k: v for k, v in fixture.items() if part(k) == which})
    for name in ("ptv1_manifest.json", "ptv1_layer.npz", "ptv1_model.npz", "ptv1_model_eval.npz", "ptv1_model_grads_enc.npz",
                 "ptv1_model_grads_dec.npz"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
