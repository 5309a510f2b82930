"""tests/golden/make_golden_refine.py -- tests/golden/refine.npz: what the reference's epoch-end label refinement computes
for the seeded rooms of tests/refine_cases.py, produced by EXECUTING the reference's own statements.  Nothing here is read at
test time except the file it writes.

pointcept/engines/train_sam_real.py cannot be imported (it needs the whole training stack, SAM and a GPU), and the
refinement is the body of one long method.  So this script reads the file at generation time, takes line ranges of it,
dedents them and `exec`s them in a namespace that holds `np`, `math`, `softmax` (scipy.special), `stats` (scipy.stats) and
the synthetic arrays under the names the reference uses.  Every range is checked for a token it must contain, so that a
reference file whose lines have moved fails here instead of executing other lines.  No line of it is copied into this
repository.

    333-338            seg_pred, confidence
    347-391            vote, the grid search, prompt_cls / prompt_idx      (347 builds 13 columns whatever the class count:
                                                                            for the 20-class room this script widens it)
    411-412, 415-416,
    418, 420-421       which points and which prompts a view sees
    453-472            the mask loop: mode and vote
    488-489, 499-500,
    510-512            the result, the check against the network, the label rewrite and count_updated

The statements between them (file I/O, SAM, logging, the two `if`s at :397 and :419 and `flag_updated` at :431) are restated
below as plain control flow.

The script also checks the CONDITIONS under which the reference alone is unambiguous, and fails otherwise (they are
conditions on the inputs, not measurements): no confidence within 1e-4 of the threshold; in every (cell, class) group the
winner and the runner-up are bit-identical logit rows or differ by more than 1e-5 in float64; the two most frequent classes
of a mask's histogram are tied exactly or differ by at least one vote.  And it measures `conf_spread`: the distance of the
reference's fp32 confidence from the float64 softmax margin of the same rows, the scale to which a device confidence is held.

usage:  python tests/golden/make_golden_refine.py <reference root>
"""
import math
import os
import sys
import textwrap

import numpy as np
from scipy import stats
from scipy.special import softmax

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import refine_cases as RC  # noqa: E402
from tests import refine_ref as RR  # noqa: E402

RANGES = {  # name: (first line, last line, a token the range must hold)
    "confidence": (333, 338, "top_two"),
    "prompts": (347, 391, "grid_scale = 0.5"),
    "view_a": (411, 412, "idx_viewable"),
    "view_b": (415, 416, "confidence_viewable"),
    "view_c": (418, 418, "prompt_viewable"),
    "view_d": (420, 421, "viewable_prompt_cls"),
    "masks": (453, 472, "stats.mode"),
    "result": (488, 489, "sam_result"),
    "check": (499, 500, "mask_check_by_model"),
    "rewrite": (510, 512, "count_updated"),
}


def load_ranges(ref):
    with open(os.path.join(ref, "pointcept", "engines", "train_sam_real.py")) as f:
        lines = f.read().split("\n")
    code = {}
    for name, (first, last, token) in RANGES.items():
        text = textwrap.dedent("\n".join(lines[first - 1:last]))
        assert token in text, "train_sam_real.py:%d-%d does not hold `%s`: the reference has moved" % (first, last, token)
        code[name] = compile(text, "train_sam_real.py:%d-%d" % (first, last), "exec")
    return code


def run_case(code, tag):
    case = RC.room(tag)
    c = case["c"]
    ns = dict(np=np, math=math, softmax=softmax, stats=stats, seg_logit=case["logits"].copy(), coord=case["coord"],
              sam_label_ori=case["label"].copy(), cls_gt_now=case["classes"], count_updated=0)
    exec(code["confidence"], ns)
    exec(code["prompts"], ns)
    if c != 13:
        ns["vote"] = np.zeros((case["n"], c), ns["sam_label_ori"].dtype)
    flag_updated, seen, hists = False, [], []
    if ns["prompt_idx"].shape[0] > 0:  # :397
        for view, bridge in enumerate(case["bridges"]):
            ns["bridge"] = bridge
            for name in ("view_a", "view_b", "view_c"):
                exec(code[name], ns)
            seen.append(int(ns["prompt_viewable"].sum()))
            if ns["prompt_viewable"].sum() > 0:  # :419
                exec(code["view_d"], ns)
                flag_updated = True  # :431
                masks = RC.masks_for(case, view, ns["viewable_prompt_coord"], ns["viewable_prompt_cls"])
                ns["masks"] = masks[:, None].copy()  # the predictor returns (P, masks per prompt, H, W); m[0] is used
                exec(code["masks"], ns)
                rows, inside = RR.inside_points(bridge, masks)
                hot = ns["confidence"][rows] > 0.9
                hists += [np.bincount(ns["seg_pred"][rows][inside[p] & hot], minlength=c) for p in range(masks.shape[0])]
    else:
        seen = [0] * len(case["bridges"])
    if flag_updated:
        for name in ("result", "check", "rewrite"):
            exec(code[name], ns)
    out = dict(pred=ns["seg_pred"].astype(np.int32), conf=ns["confidence"], prompt_idx=ns["prompt_idx"].astype(np.int32),
               prompt_cls=ns["prompt_cls"].astype(np.int32), vote=ns["vote"].astype(np.int16),
               label=ns["sam_label_ori"][:, 0].astype(np.int32), updated=np.int64(ns["count_updated"]),
               touched=np.bool_(flag_updated), seen=np.asarray(seen, np.int32), digest=np.str_(RC.digest(case)))
    assert out["conf"].dtype == np.float32
    check_conditions(case, out, hists)
    _, conf64 = RR.confidence(case["logits"], np.float64)
    out["conf_spread"] = np.float64(np.abs(out["conf"].astype(np.float64) - conf64).max())
    return out


def check_conditions(case, out, hists):
    _, conf64 = RR.confidence(case["logits"], np.float64)
    assert np.abs(conf64 - RC.THRESHOLD).min() > 1e-4 and np.abs(out["conf"] - np.float32(RC.THRESHOLD)).min() > 1e-4
    _, _, groups = RR.prompts(case["coord"], out["pred"], out["conf"], case["label"], case["present"], RC.GRID, RC.THRESHOLD,
                              groups=True)
    ties = 0
    for rows in groups.values():
        if rows.size > 1:
            ties += np.array_equal(case["logits"][rows[0]], case["logits"][rows[1]])
            other = [r for r in rows[1:] if not np.array_equal(case["logits"][r], case["logits"][rows[0]])]
            assert not other or conf64[rows[0]] - conf64[other[0]] > 1e-5, (rows[0], other[0])
    assert ties >= 3, "the duplicated rows lead no group"
    mode_ties = 0
    for h in hists:
        top = np.sort(h)[-2:]
        assert top[1] == top[0] or top[1] - top[0] >= 1
        mode_ties += top[1] == top[0] and top[1] > 0
    print("  %s: %d prompts, %d exact ties lead a group, %d masks (%d with a tied mode), votes up to %d, %d labels updated, "
          "prompts seen per view %s" % (case["tag"], out["prompt_idx"].size, ties, len(hists), mode_ties, out["vote"].max(),
                                        out["updated"], out["seen"].tolist()))
    assert out["prompt_idx"].size > 20 and out["vote"].max() >= 2 and 0 < out["updated"] and min(out["seen"]) == 0 < max(out["seen"])


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["POINTCEPT_ROOT"]
    code = load_ranges(ref)
    fx = {}
    for tag in RC.CASES:
        for k, v in run_case(code, tag).items():
            fx["%s_%s" % (tag, k)] = v
        print("  %s: conf_spread %.3e" % (tag, fx[tag + "_conf_spread"]))
    path = os.path.join(HERE, "refine.npz")
    np.savez_compressed(path, **fx)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
