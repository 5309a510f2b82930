"""tests/golden/make_golden_lovasz.py -- regenerates tests/golden/lovasz.npz from the reference's own Lovasz loss.

Runs ONLY in the build container (it loads pointcept/models/losses/lovasz.py from /root/reference, which does not exist on
the GPU box); nothing here is read at test time except the .npz it writes.  lovasz.py is pure torch and runs unmodified
on CPU; its `from .builder import LOSSES` is stubbed with a no-op registry.

Every case stores the inputs, the reference's loss and d loss / d logits of
`LovaszLoss(mode="multiclass", ignore_index, class_seen, loss_weight)(logits, label)`.  The reference's torch.sort does not
pin the order of equal errors, so the inputs are built with errors that are far apart within every class: the rows'
probabilities are chosen (distinct grid values for the background classes, the labelled class takes the rest) and the
logits are their logarithms.  The generator asserts a gap of at least 1e-6 between any two errors of a class, so an
implementation whose softmax differs from torch's CPU one by a few ulps still sorts them in the same order.

usage:  python tests/golden/make_golden_lovasz.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
MIN_GAP = 1e-6


def load_reference():
    class _Registry:
        def register_module(self, *a, **k):
            return (lambda cls: cls) if not a or not isinstance(a[0], type) else a[0]

    for name in ("pointcept", "pointcept.models", "pointcept.models.losses"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    builder = types.ModuleType("pointcept.models.losses.builder")
    builder.LOSSES = _Registry()
    sys.modules[builder.__name__] = builder
    spec = importlib.util.spec_from_file_location("pointcept.models.losses.lovasz",
                                                  os.path.join(REF, "pointcept/models/losses/lovasz.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def separated_logits(rng, label, c, used):
    """(n, c) fp32 logits whose softmax has well separated errors |fg - p| in every class over the used rows: background
    probabilities are distinct even multiples of delta per class, a row's labelled class takes 1 - their sum, and where two
    rows of a class would get the same sum, one background entry of one of them is moved to the odd multiple above it."""
    n = len(label)
    v = np.stack([2 * rng.permutation(n) + 2 for _ in range(c)], 1).astype(np.int64)
    y = np.where(used, label, 0)
    v[np.arange(n), y] = 0
    for k in range(c):
        rows = np.flatnonzero(used & (label == k))
        while True:
            sums = v[rows].sum(1)
            _, first = np.unique(sums, return_index=True)
            dup = np.setdiff1d(np.arange(len(rows)), first)
            if not len(dup):
                break
            for i in rows[dup]:
                j = rng.choice(np.flatnonzero((v[i] % 2 == 0) & (np.arange(c) != k)))
                v[i, j] += 1
    delta = 0.9 / ((c - 1) * (2 * n + 2))
    q = v * delta
    q[np.arange(n), y] = 1.0 - q.sum(1)
    return np.log(q).astype(np.float32)


def min_gap(logits, label, c, used):
    p = torch.softmax(torch.from_numpy(logits), 1).numpy()
    gaps = []
    for k in range(c):
        fg = (label[used] == k).astype(np.float32)
        e = np.sort(np.abs(fg - p[used, k]))
        if len(e) > 1:
            gaps.append(float(np.diff(e).min()))
    return min(gaps) if gaps else 1.0


def case(ref, rng, n, c, ignore_index, ignore_frac, classes=None, class_seen=None, loss_weight=1.0, labelled=None):
    for _ in range(100):
        label = rng.choice(classes if classes is not None else np.arange(c), size=n).astype(np.int64)
        if labelled is not None:
            keep = np.zeros(n, bool)
            keep[rng.choice(n, labelled, replace=False)] = True
            label[~keep] = ignore_index
        elif ignore_frac:
            label[rng.random(n) < ignore_frac] = ignore_index
        used = label != ignore_index
        logits = separated_logits(rng, label, c, used)
        if min_gap(logits, label, c, used) >= MIN_GAP:
            break
    else:
        raise RuntimeError("no well separated draw")
    x = torch.from_numpy(logits).requires_grad_(True)
    crit = ref.LovaszLoss(mode="multiclass", class_seen=class_seen, ignore_index=ignore_index, loss_weight=loss_weight)
    loss = crit(x, torch.from_numpy(label))
    loss.backward()
    return dict(logits=logits, label=label.astype(np.int32), loss=np.float32(loss.detach()), grad=x.grad.numpy(),
                ignore_index=np.int64(ignore_index), loss_weight=np.float32(loss_weight),
                class_seen=np.asarray([] if class_seen is None else class_seen, np.int64),
                has_class_seen=np.int64(class_seen is not None))


def main():
    ref = load_reference()
    rng = np.random.default_rng(20)
    cases = {
        "c20": case(ref, rng, 4096, 20, -1, 0.1),
        "c20seen": None,
        "c13absent": case(ref, rng, 2048, 13, -1, 0.05, classes=np.array([0, 1, 2, 4, 5, 7, 8, 11])),
        "w05_i255": case(ref, rng, 2048, 13, 255, 0.1, loss_weight=0.5),
        "one_row": case(ref, rng, 64, 20, -1, 0.0, labelled=1),
    }
    # the first case's inputs again, averaged over class_seen only (and a class id outside [0, C), ignored as by the reference)
    base = cases["c20"]
    x = torch.from_numpy(base["logits"]).requires_grad_(True)
    seen = [0, 2, 3, 5, 7, 11, 13, 17, 19, 25]
    loss = ref.LovaszLoss(mode="multiclass", class_seen=seen, ignore_index=-1)(x, torch.from_numpy(base["label"].astype(np.int64)))
    loss.backward()
    cases["c20seen"] = dict(loss=np.float32(loss.detach()), grad=x.grad.numpy(), ignore_index=np.int64(-1),
                            loss_weight=np.float32(1.0), class_seen=np.asarray(seen, np.int64), has_class_seen=np.int64(1),
                            inputs_of=np.array("c20"))
    out = {}
    for name, d in cases.items():
        for k, v in d.items():
            out["%s__%s" % (name, k)] = v
    out["cases"] = np.array(list(cases))
    path = os.path.join(HERE, "lovasz.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(d["loss"]) for k, d in cases.items()})


if __name__ == "__main__":
    main()
