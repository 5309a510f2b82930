"""tests/golden/make_golden_cac.py -- regenerates tests/golden/cac.npz from the reference's own CAC-v1m1 segmentor.

Runs ONLY in the build container (it loads pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py
and pointcept/models/losses/{builder,misc,lovasz}.py from /root/reference, which does not exist on the GPU box); nothing
here is read at test time except the .npz it writes.  The registries are stubbed, `Tensor.cuda` is the identity inside this
script only (the reference calls `.cuda()` on fresh tensors), and the backbone is a stub that returns the case's leaf `feat`.

Every case runs one training step (forward, the five loss terms, backward) and then an eval-mode forward with `segment`, and
stores: the inputs (the head parameters before the step are shared by the cases of a class count, `param_k<K>/`; they
and `feat` hold fp16-exact values, stored as fp16), the five loss terms, d loss / d feat, every head parameter's
gradient, the BatchNorm running statistics and num_batches_tracked after the step, the eval-mode seg_logits and loss, and the
state_dict key list.  Lovasz sorts errors: for the CE + Lovasz cases the seed is advanced until, in each of the three logit
sets the criteria see, the errors |fg - p| of every present class are at least MIN_GAP apart.

usage:  python tests/golden/make_golden_cac.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
MIN_GAP = 3e-6
C = 48

CE = dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)
LOV = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)
# name: (K, rows per scene, conf_thresh, detach_pre_logits, criteria, absent classes)
CASES = {
    "k20_t075_det_celov": (20, (70, 50), 0.75, True, [CE, LOV], (3, 7)),
    "k200_t0_det_celov": (200, (50, 40), 0.0, True, [CE, LOV], ()),
    "k20_t0_nodet_ce": (20, (100, 80), 0.0, False, [CE], (5,)),
    "k20_t075_nodet_ce": (20, (90, 70), 0.75, False, [CE], (0, 11)),
}


class _Registry:
    def __init__(self, name=""):
        self._d = {}

    def register_module(self, name=None, module=None, force=False):
        def deco(cls):
            self._d[name or cls.__name__] = cls
            return cls
        return deco(module) if module is not None else deco

    def build(self, cfg):
        cfg = dict(cfg)
        return self._d[cfg.pop("type")](**cfg)


class StubBackbone(nn.Module):
    def forward(self, data_dict):
        return data_dict["feat"]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("pointcept", "pointcept.utils", "pointcept.models", "pointcept.models.losses",
                 "pointcept.models.context_aware_classifier"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    reg = types.ModuleType("pointcept.utils.registry")
    reg.Registry = _Registry
    sys.modules[reg.__name__] = reg
    builder = _load("pointcept.models.losses.builder", "pointcept/models/losses/builder.py")
    _load("pointcept.models.losses.misc", "pointcept/models/losses/misc.py")
    _load("pointcept.models.losses.lovasz", "pointcept/models/losses/lovasz.py")
    sys.modules["pointcept.models.losses"].build_criteria = builder.build_criteria
    mb = types.ModuleType("pointcept.models.builder")
    mb.MODELS = _Registry("models")
    mb.build_model = lambda cfg: StubBackbone()
    sys.modules[mb.__name__] = mb
    return _load("pointcept.models.context_aware_classifier.context_aware_classifier_v1m1_base",
                 "pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py")


def make_inputs(seed, k, rows, absent):
    g = torch.Generator().manual_seed(seed)
    n = sum(rows)
    feat = torch.randn(n, C, generator=g) * 2.0
    label = torch.randint(0, k, (n,), generator=g)
    for a in absent:
        label[label == a] = (a + 1) % k
    label[torch.rand(n, generator=g) < 0.12] = -1
    offset = torch.tensor(np.cumsum(rows), dtype=torch.int64)
    return feat, label, offset


def min_gap(logits, label):
    """smallest distance between two errors of a present class whose order changes the Lovasz gradient"""
    p = torch.softmax(logits.detach().double(), 1)
    used = label != -1
    gap = float("inf")
    for c in label[used].unique().tolist():
        fg = (label[used] == c).double()
        e, order = torch.sort((fg - p[used, c]).abs(), descending=True)
        # past the last foreground row the Lovasz gradient is 0 whatever the order: only the head of the order counts
        last = int(torch.nonzero(fg[order]).max()) + 2
        e = e[:last]
        if len(e) > 1:
            gap = min(gap, float((e[:-1] - e[1:]).min()))
    return gap


def head_state(ref, k):
    """one parameter set per class count, shared by its cases; values exactly representable in fp16 (stored as such)"""
    torch.manual_seed(7 + k)
    model = ref.CACSegmentor(num_classes=k, backbone_out_channels=C, backbone=dict(type="stub"))
    with torch.no_grad():  # seg_head rows large enough that some rows pass the confidence threshold
        model.seg_head.weight.mul_(2.5)
        bn = model.feat_proj_layer[1]
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
        for v in model.state_dict().values():
            if v.is_floating_point():
                v.copy_(v.half().float())
    return {kk: v.detach().clone() for kk, v in model.state_dict().items()}


def run_case(ref, name, k, rows, thr, detach, criteria, absent, seed):
    state0 = head_state(ref, k)
    model = ref.CACSegmentor(num_classes=k, backbone_out_channels=C, backbone=dict(type="stub"), criteria=criteria,
                             conf_thresh=thr, detach_pre_logits=detach)
    model.load_state_dict(state0)
    feat, label, offset = make_inputs(seed, k, rows, absent)
    feat = feat.half().float()
    leaf = feat.clone().requires_grad_(True)
    model.train()
    data = dict(feat=leaf, offset=offset, segment=label)
    if any(c["type"] == "LovaszLoss" for c in criteria):
        with torch.no_grad():
            m2 = ref.CACSegmentor(num_classes=k, backbone_out_channels=C, backbone=dict(type="stub"), criteria=criteria,
                                  conf_thresh=thr, detach_pre_logits=detach)
            m2.load_state_dict(state0)
            m2.train()
            f = feat
            seg = m2.seg_head(f)
            refine = m2.post_refine_proto_batch(feat=f, pred=seg, proto=m2.seg_head.weight.squeeze(), offset=offset) * m2.cos_temp
            cac = m2.get_adaptive_perspective(feat=f, target=label, new_proto=m2.seg_head.weight.detach().data.squeeze(),
                                              proto=m2.seg_head.weight.squeeze()) * m2.cos_temp
            gap = min(min_gap(seg, label), min_gap(refine, label), min_gap(cac, label))
        if gap < MIN_GAP:
            return None
    out = model(data)
    out["loss"].backward()
    rec = {"feat": feat.half().numpy(), "segment": label.numpy(), "offset": offset.numpy(),
           "config": np.array([k, C, thr, float(detach), float(len(criteria) > 1), model.cos_temp], np.float64)}
    for t in ("loss", "seg_loss", "pre_loss", "pre_self_loss", "kl_loss"):
        rec["out/" + t] = np.float64(float(out[t].detach()))
    rec["grad/feat"] = leaf.grad.numpy()
    for kk, p in model.named_parameters():
        rec["grad/" + kk] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    for kk, v in model.state_dict().items():
        if "running" in kk or "num_batches" in kk:
            rec["after/" + kk] = v.numpy()
    model.eval()
    with torch.no_grad():
        ev = model(dict(feat=feat, offset=offset, segment=label))
    rec["eval/seg_logits"] = ev["seg_logits"].numpy()
    rec["eval/loss"] = np.float64(float(ev["loss"]))
    rec["keys"] = np.array(list(model.state_dict().keys()))
    return rec


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_num_threads(4)
    ref = load_reference()
    out = {}
    for k in sorted({v[0] for v in CASES.values()}):
        for kk, v in head_state(ref, k).items():
            out["param_k%d/%s" % (k, kk)] = v.half().numpy() if v.is_floating_point() else v.numpy()
    for name, (k, rows, thr, detach, criteria, absent) in CASES.items():
        for seed in range(100, 400):
            rec = run_case(ref, name, k, rows, thr, detach, criteria, absent, seed)
            if rec is not None:
                break
        else:
            raise RuntimeError("no seed separates the Lovasz errors of " + name)
        print(name, "seed", seed, "loss", float(rec["out/loss"]))
        for kk, v in rec.items():
            out[name + "/" + kk] = v
    path = os.path.join(HERE, "cac.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
