"""Generates the PT-v2m1 fixtures from the REFERENCE model, unmodified, on CPU torch.

    python -m tests.golden.make_golden_ptv2m1

Runs only where the reference checkout is present (make_golden.REF).  What is executed from the reference: its module
pointcept/models/point_transformer_v2/point_transformer_v2m1_origin.py (GroupedLinear, GroupedVectorAttention,
PointTransformerV2) over the oracle-backed `pointops` and the stubs of tests/golden/make_golden.py::install_stubs, and the
`model = dict(...)` statement of the three PT-v2m1 configs (for the backbone keywords).  No reference text is copied.

Writes
  tests/golden/ptv2m1_manifest.json   for s3dis / scannet / scannet200: the backbone keywords ("<tag>_cfg"), state-dict keys and
                                      shapes ("<tag>"; scannet200 as "scannet200_except", what differs from scannet), the
                                      parameter count ("<tag>_num_params")
  tests/golden/ptv2m1.npz             model_*: the small model of tests/ptv2m1_cases.py::MODEL_CFG (drop_path 0) on two clouds:
                                      logits and loss in train and eval mode, EVERY parameter gradient of the training loss, the
                                      running buffers after that one training forward;
                                      attn<C>_*: one GroupedVectorAttention (pe_multiplier, pe_bias) per (C, G) on two clouds
                                      shorter than k (-1 slots in every row): output in train and eval mode, the input gradient,
                                      the gradients of the narrow parameters, the running buffers.
The weights are not stored: both sides draw them with tests/ptv2m1_cases.py::init_state; the file holds their digests."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import ptv2m1_cases as C  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402

CONFIGS = (("s3dis", "configs/s3dis/semseg-pt-v2m1-0-base.py"), ("scannet", "configs/scannet/semseg-pt-v2m1-0-origin.py"),
           ("scannet200", "configs/scannet200/semseg-pt-v2m1-0-base.py"))
# parameters of an attention module whose gradients fit a fixture (the C x C ones are checked through the model case)
NARROW = ("weight_encoding.0.weight", "weight_encoding.3.weight", "weight_encoding.1.norm.weight", "linear_p_multiplier.0.weight",
          "linear_p_multiplier.1.norm.weight", "linear_p_multiplier.3.bias", "linear_p_bias.0.weight", "linear_p_bias.3.bias")


def load_reference():
    spec = importlib.util.spec_from_file_location(
        "ref_ptv2m1", os.path.join(MG.REF, "pointcept/models/point_transformer_v2/point_transformer_v2m1_origin.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def backbone_cfg(path):
    # (the scannet200 config imports its class names from a constants module of the reference: loaded by path, its parent
    # packages as empty modules -- `pointcept` itself is never imported as a package here)
    name = "pointcept.datasets.preprocessing.scannet.meta_data.scannet200_constants"
    if name not in sys.modules:
        parts = name.split(".")
        for i in range(1, len(parts)):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        spec = importlib.util.spec_from_file_location(name, os.path.join(MG.REF, name.replace(".", "/") + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules[name] = mod
    ns = {}
    with open(os.path.join(MG.REF, path)) as f:
        exec(compile(f.read(), path, "exec"), ns)
    cfg = dict(ns["model"]["backbone"])
    assert cfg.pop("type") == "PT-v2m1"
    return cfg


def write_manifest(man):
    """One line per entry; scannet200 as what differs from scannet ("scannet200_except": the classifier's last layer), so that
    the file stays a few lines of a size a reader can scan."""
    man = dict(man)
    full = man.pop("scannet200")
    assert set(full) == set(man["scannet"])
    man["scannet200_except"] = {k: v for k, v in full.items() if man["scannet"][k] != v}
    with open(os.path.join(HERE, "ptv2m1_manifest.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(man[k], sort_keys=True, separators=(",", ":")))
                                  for k in sorted(man)) + "\n}\n")


def gen_manifest(ref):
    man = {}
    for tag, path in CONFIGS:
        cfg = backbone_cfg(path)
        model = ref.PointTransformerV2(**dict(cfg, drop_path_rate=0.0))  # (DropPath has no parameters; the stub takes 0 only)
        man[tag + "_cfg"] = cfg
        man[tag] = {k: list(v.shape) for k, v in model.state_dict().items()}
        man[tag + "_num_params"] = sum(p.numel() for p in model.parameters())
    write_manifest(man)
    print("manifest:", {k: (len(v) if isinstance(v, dict) else v) for k, v in man.items() if not k.endswith("_cfg")})


def gen_model(ref, out):
    model = ref.PointTransformerV2(**C.MODEL_CFG)
    st = C.init_state({k: v.shape for k, v in model.state_dict().items()}, C.MODEL_SEED)
    coord, offset, feat, label = C.model_inputs()
    out["model_digest"] = C.state_digest(st)
    for mode in ("train", "eval"):
        model.load_state_dict(st, strict=True)
        model.train(mode == "train")
        logits = model(dict(coord=coord, feat=feat, offset=offset))
        loss = torch.nn.functional.cross_entropy(logits, label, ignore_index=-1)
        out["model_logits_" + mode], out["model_loss_" + mode] = logits, loss
        if mode == "train":
            names = [n for n, _ in model.named_parameters()]
            for n, gr in zip(names, torch.autograd.grad(loss, list(model.parameters()))):
                out["model_grad_" + n] = gr
            for n, b in model.named_buffers():
                if n.endswith(("running_mean", "running_var")):
                    out["model_buf_" + n] = b.clone()


def gen_modules(ref, out):
    import pointops

    for c, g in C.SHAPES:
        coord, offset, feat0, gout = C.module_inputs(c)
        idx, _ = pointops.knn_query(16, coord, offset)
        assert int((idx < 0).sum()) >= idx.shape[0]
        attn = ref.GroupedVectorAttention(embed_channels=c, groups=g, pe_multiplier=True, pe_bias=True)
        st = C.init_state({k: v.shape for k, v in attn.state_dict().items()}, C.MODULE_SEED + c)
        tag = "attn%d_" % c
        out[tag + "digest"], out[tag + "idx"] = C.state_digest(st), idx
        for mode in ("train", "eval"):
            attn.load_state_dict(st, strict=True)
            attn.train(mode == "train")
            feat = feat0.clone().requires_grad_(True)
            y = attn(feat, coord, idx)
            out[tag + "out_" + mode] = y
            if mode == "train":
                params = dict(attn.named_parameters())
                grads = torch.autograd.grad(y, [feat] + [params[n] for n in NARROW], gout)
                out[tag + "gfeat"] = grads[0]
                for n, gr in zip(NARROW, grads[1:]):
                    out[tag + "g_" + n] = gr
                for n, b in attn.named_buffers():
                    if n.endswith(("running_mean", "running_var")) and (n.startswith("linear_p") or n.startswith("weight_encoding")):
                        out[tag + "buf_" + n] = b.clone()


def main():
    assert os.path.isdir(MG.REF), "needs the reference checkout"
    MG.install_stubs()
    ref = load_reference()
    gen_manifest(ref)
    out = {}
    gen_model(ref, out)
    gen_modules(ref, out)
    MG.save("ptv2m1.npz", **out)
    print("ptv2m1.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "ptv2m1.npz")))


if __name__ == "__main__":
    main()
