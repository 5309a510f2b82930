"""tests/golden/make_golden_inseval.py -- the instance-evaluator fixture, produced by RUNNING the reference's InsSegEvaluator on the
CPU over the scenes of tests/inseval_cases.py:

    inseval.npz   per scene the inputs (masks as int8 bytes stored uint8), the reference's gt / pred dict lists flattened to the
                  arrays of a SceneMatches record, and for the four scenes together `ap_scores` and the classes x overlaps table

The reference's pointcept/engines/hooks/evaluator.py is imported by path under five stub modules (pointops, pointcept.utils.comm,
pointcept.utils.misc, .default with HookBase, .builder with HOOKS); the hook gets a stub trainer whose cfg.data carries the names
and the number of classes.  The reference intersects a proposal only with the ground truths of the proposal's own class; the
record holds every pair, so `associate_instances` is run once more per class with every proposal given that class, and the
columns of that class are taken from that run.  The table comes from `evaluate_matches` with overlaps = [x, 0.25] for each x.
Only data is written.

usage:  python tests/golden/make_golden_inseval.py <reference root>
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import inseval_cases as C  # noqa: E402


def load_reference(ref):
    class Registry:
        def register_module(self, *args, **kwargs):
            return lambda cls: cls

    def module(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    module("pointops")
    folder = os.path.join(ref, "pointcept", "engines", "hooks")
    for name in ("pointcept", "pointcept.utils", "pointcept.engines", "pointcept.engines.hooks"):
        module(name).__path__ = []
    module("pointcept.utils.comm")
    module("pointcept.utils.misc", intersection_and_union_gpu=None)
    module("pointcept.engines.hooks.default", HookBase=type("HookBase", (), {"trainer": None}))
    module("pointcept.engines.hooks.builder", HOOKS=Registry())
    name = "pointcept.engines.hooks.evaluator"
    spec = importlib.util.spec_from_file_location(name, os.path.join(folder, "evaluator.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.InsSegEvaluator


def make_hook(cls):
    hook = cls(segment_ignore_index=C.SEGMENT_IGNORE, instance_ignore_index=C.INSTANCE_IGNORE)
    data = types.SimpleNamespace(names=C.NAMES, num_classes=C.NUM_CLASSES)
    hook.trainer = types.SimpleNamespace(cfg=types.SimpleNamespace(data=data))
    hook.before_train()
    assert hook.min_region_sizes == C.MIN_REGION
    return hook


def run_scene(hook, scene, classes=None):
    pred = dict(pred_masks=torch.from_numpy(scene["masks"]), pred_scores=torch.from_numpy(scene["scores"]),
                pred_classes=torch.from_numpy(scene["classes"] if classes is None else classes))
    return hook.associate_instances(pred, torch.from_numpy(scene["segment"]), torch.from_numpy(scene["instance"]))


def flatten(hook, scene, gt, pred):
    """the reference's per-class dict lists as the arrays of the record"""
    gts = sorted((g for name in gt for g in gt[name]), key=lambda g: int(g["instance_id"]))
    preds = sorted((p for name in pred for p in pred[name]), key=lambda p: int(p["instance_id"]))
    assert [int(p["instance_id"]) for p in preds] == list(range(len(preds)))
    # the row of each kept proposal: the reference numbers them in row order, so walk the rows
    rows, row = [], 0
    for p in preds:
        while not (np.array_equal(p["mask"], scene["masks"][row] != 0) and int(p["segment_id"]) == int(scene["classes"][row])
                   and scene["classes"][row] not in C.SEGMENT_IGNORE):
            row += 1
        rows.append(row)
        row += 1
    col = {int(g["instance_id"]): i for i, g in enumerate(gts)}
    inter = np.zeros((len(preds), len(gts)), np.int64)
    for q, p in enumerate(preds):
        for g in p["matched_gt"]:
            assert int(g["segment_id"]) == int(p["segment_id"]) and g["intersection"] > 0
            inter[q, col[int(g["instance_id"])]] = g["intersection"]
    # the other classes' columns: every proposal given class c, the reference run again
    for c in sorted({int(g["segment_id"]) for g in gts}):
        as_c = np.where(np.isin(scene["classes"], C.SEGMENT_IGNORE), scene["classes"], c)
        _, pred_c = run_scene(hook, scene, as_c)
        assert [n for n in pred_c if pred_c[n]] == [C.NAMES[c]] or not preds
        for q, p in enumerate(sorted(pred_c[C.NAMES[c]], key=lambda p: int(p["instance_id"]))):
            assert np.array_equal(p["mask"], preds[q]["mask"])
            for i, g in enumerate(gts):
                if int(g["segment_id"]) == c:
                    got = [m["intersection"] for m in p["matched_gt"] if int(m["instance_id"]) == int(g["instance_id"])]
                    value = got[0] if got else 0
                    assert int(preds[q]["segment_id"]) != c or inter[q, i] == value
                    inter[q, i] = value
    return dict(gt_instance_id=np.array([int(g["instance_id"]) for g in gts], np.int64),
                gt_segment_id=np.array([int(g["segment_id"]) for g in gts], np.int64),
                gt_vert_count=np.array([int(g["vert_count"]) for g in gts], np.int64), pred_row=np.array(rows, np.int64),
                pred_class=np.array([int(p["segment_id"]) for p in preds], np.int64),
                pred_conf=np.array([float(p["confidence"]) for p in preds], np.float64),
                pred_vert_count=np.array([int(p["vert_count"]) for p in preds], np.int64),
                pred_void=np.array([int(p["void_intersection"]) for p in preds], np.int64), inter=inter)


def main():
    hook = make_hook(load_reference(sys.argv[1]))
    out, recorded = {}, []
    for name, scene in C.scenes().items():
        gt, pred = run_scene(hook, scene)
        recorded.append(dict(gt=gt, pred=pred))
        for key, value in scene.items():
            out["%s.%s" % (name, key)] = value.astype(np.int8).view(np.uint8) if key == "masks" else value
        for key, value in flatten(hook, scene, gt, pred).items():
            out["%s.record.%s" % (name, key)] = value
    valid = [i for i in range(C.NUM_CLASSES) if i not in C.SEGMENT_IGNORE]
    assert hook.valid_class_names == [C.NAMES[i] for i in valid]
    overlaps = hook.overlaps.copy()
    with np.errstate(all="ignore"):
        scores = hook.evaluate_matches(recorded)
        table = np.zeros((len(valid), len(overlaps)))
        for oi, x in enumerate(overlaps[:-1]):
            hook.overlaps = np.array([x, 0.25])
            part = hook.evaluate_matches(recorded)
            for li, label in enumerate(hook.valid_class_names):
                table[li, oi] = part["classes"][label]["ap"]
                table[li, -1] = part["classes"][label]["ap25%"]
        hook.overlaps = overlaps
    out["overlaps"], out["valid_class_ids"], out["ap_table"] = overlaps, np.array(valid, np.int64), table
    for key in ("all_ap", "all_ap_50%", "all_ap_25%"):
        out["ap_scores." + key] = np.float64(scores[key])
    for key in ("ap", "ap50%", "ap25%"):
        out["ap_scores.classes." + key] = np.array([scores["classes"][n][key] for n in hook.valid_class_names], np.float64)
    path = os.path.join(HERE, "inseval.npz")
    np.savez_compressed(path, **out)
    print("inseval.npz", os.path.getsize(path), "bytes;", {k: out[k] for k in out if k.startswith("ap_scores.")})
    print(np.round(table, 4))


if __name__ == "__main__":
    import warnings

    warnings.simplefilter("ignore", RuntimeWarning)  # (nanmean of the all-NaN classes)
    main()
