"""tests/golden/make_golden_pp2s.py -- tests/golden/pp2s.npz: what the reference's three PP2S scripts compute for the seeded
rooms of tests/pp2s_cases.py, produced by EXECUTING the reference's own statements.  Nothing here is read at test time
except the file it writes.

The scripts (pointcept/utils/my_make_bridge_final.py, my_choose_weak_label_final.py, my_run_sam_final.py) cannot be imported:
they are module-level loops over a dataset on disk and need SAM.  So this script reads the files at generation time, takes
line ranges of them, dedents them and `exec`s them in a namespace that holds `np` and the synthetic arrays under the names
the scripts use.  Every range is checked for a token it must contain, so that a reference file whose lines have moved fails
here instead of executing other lines.  No line of them is copied into this repository.

    my_make_bridge_final.py         89-96     the angle, the rotation matrix, the alignment
                                    124-153   one view: bounds, projection, depth test, bridge, viewable_all
    my_choose_weak_label_final.py   59-60     viewable_all, weak_mask
                                    67-68     one bridge file's visible points
                                    71-88     one weak point per instance
    my_run_sam_final.py             83-114    one frame: the prompts it sees, a mask per prompt, the vote table
                                    117-122   the weak points are written over with their ground truth

The statements between them (file and image I/O, the loops over areas, rooms and frames, `sam_label_pcd` and `mask_dict` of
:71-74) are restated below as plain control flow; `sam_predictor` and `frame_embed` are stubs in the namespace (the stub's
masks are tests/pp2s_cases.masks_for), `rgb_path` a string, `print` silent.  A bridge exists for a view exactly when :148
ran, as :155 saves it there.

The script also checks the CONDITIONS under which the reference alone is unambiguous, and fails otherwise (they are
conditions on the inputs, not measurements): no projected coordinate within 1e-6 of a half-integer or of a bound, no
|depth - z_cam| within 1e-6 of 0.1, no p.z within 1e-6 of 0.  Everything after the projection is integer.

usage:  python tests/golden/make_golden_pp2s.py <reference root>
"""
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import pp2s_cases as PC  # noqa: E402
from tests import pp2s_ref as PR  # noqa: E402

RANGES = {  # name: (file, first line, last line, a token the range must hold)
    "align": ("my_make_bridge_final.py", 89, 96, "coord -= room_center"),
    "view": ("my_make_bridge_final.py", 124, 153, "viewable_idx_"),
    "weak_init": ("my_choose_weak_label_final.py", 59, 60, "weak_mask"),
    "weak_bridge": ("my_choose_weak_label_final.py", 67, 68, "viewable_all[viewable_idx]"),
    "weak_choose": ("my_choose_weak_label_final.py", 71, 88, "idx_weak"),
    "frame": ("my_run_sam_final.py", 83, 114, "valid_point_list"),
    "overwrite": ("my_run_sam_final.py", 117, 122, "semantic_gt"),
}
MARGIN = 1e-6


def load_ranges(ref):
    code = {}
    for name, (file, first, last, token) in RANGES.items():
        with open(os.path.join(ref, "pointcept", "utils", file)) as f:
            lines = f.read().split("\n")
        text = textwrap.dedent("\n".join(lines[first - 1:last]))
        assert token in text, "%s:%d-%d does not hold `%s`: the reference has moved" % (file, first, last, token)
        code[name] = compile(text, "%s:%d-%d" % (file, first, last), "exec")
    return code


class Predictor:
    """sam_predictor: one mask per call, the seeded disc of the prompt the frame loop is at"""

    def __init__(self, case, ns):
        self.case, self.ns, self.features, self.calls = case, ns, None, {}

    def predict(self, point_coords, point_labels):
        assert point_coords.shape == (1, 2) and point_labels.tolist() == [1]
        at = int(self.ns["prompt_number"])
        cls = int(self.case["semantic"][at, 0])
        self.calls.setdefault(self.ns["view_key"], []).append((at, int(point_coords[0, 0]), int(point_coords[0, 1]), cls))
        return PC.masks_for(self.case, self.ns["view_key"], point_coords, [cls]), None, None


class Embedding:
    def cuda(self):
        return self


def run_case(code, tag):
    case = PC.room(tag)
    n = case["n"]
    quiet = lambda *a, **k: None  # noqa: E731
    # ---- my_make_bridge_final.py
    ns = dict(np=np, print=quiet, coord=case["coord"].copy(), room_str="room", center_dict={"room": case["center"].copy()},
              aa_dict={"room": int(case["angle"])}, viewable_all=np.zeros(n, np.int64))
    exec(code["align"], ns)
    aligned = ns["coord"]
    assert aligned.dtype == np.float64
    saved, visible, margins = {}, [], dict(half=np.inf, bound=np.inf, gap=np.inf, pz=np.inf)
    for view in case["views"]:
        ns.pop("bridge", None)
        ns.update(rgb_path=view["key"], depth=view["depth"] / 512, k_matrix=view["k"], rt_matrix=view["rt"])  # (:118)
        exec(code["view"], ns)
        if "bridge" in ns:
            assert ns["bridge"].dtype == np.uint16
            saved[view["key"]] = ns["bridge"]
        visible.append(int(ns["bridge"][:, 2].sum()) if "bridge" in ns else 0)
        m = PR.project(aligned, view["k"], view["rt"], view["depth"] / PC.DEPTH_SCALE, PC.TOL, margins=True)[3]
        margins = {k: min(margins[k], m[k]) for k in margins}
    assert min(margins.values()) > MARGIN, margins
    # ---- my_choose_weak_label_final.py
    ns = dict(np=np, label_instance=case["instance"].reshape(-1), label_segment=case["semantic"].reshape(-1))
    exec(code["weak_init"], ns)
    for key in sorted(saved):
        ns["bridge"] = saved[key]
        exec(code["weak_bridge"], ns)
    exec(code["weak_choose"], ns)
    seen_any, weak = ns["viewable_all"].astype(np.uint8), ns["weak_mask"].astype(np.uint8)
    # ---- my_run_sam_final.py
    ns = dict(np=np, prompt=weak, pcd_data={"semantic_gt": case["semantic"]}, mask_num=0, mask_dict=dict(), frame_embed=Embedding(),
              sam_label_pcd=(-1 * np.ones((n, 1))).astype(np.int32), scene_pcd_np=case["coord"])
    ns["sam_predictor"] = predictor = Predictor(case, ns)
    votes = []
    for key in sorted(saved):  # (a room without frames, :47-60, does what `overwrite` does on labels of -1)
        ns.update(view_key=key, frame_bridge=saved[key].copy())
        exec(code["frame"], ns)
        votes.append({p: set(d) for p, d in ns["mask_dict"].items()})
    before = ns["sam_label_pcd"].copy()
    exec(code["overwrite"], ns)
    label = ns["sam_label_pcd"]
    assert label.dtype == np.int32 and label.shape == (n, 1)

    out = dict(aligned=aligned[::PC.ALIGN_STRIDE], visible=np.asarray(visible, np.int32), seen_any=np.packbits(seen_any),
               weak=np.nonzero(weak)[0].astype(np.int32), label=label[:, 0].astype(np.int8), digest=np.str_(PC.digest(case)))
    for v, view in enumerate(case["views"]):
        bridge = saved.get(view["key"], np.zeros((n, 3), np.uint16))
        rows = np.nonzero(bridge[:, 2])[0]
        out["bridge%d" % v] = np.concatenate([rows[:, None], bridge[rows, :2]], 1).astype(np.uint16)  # (row, x, y) of the visible
        out["prompts%d" % v] = np.asarray(predictor.calls.get(view["key"], []), np.int32).reshape(-1, 4)  # (idx, x, y, class)
    check_coverage(case, out, saved, seen_any, weak, before[:, 0], label[:, 0], votes, margins)
    return out


def check_coverage(case, out, saved, seen_any, weak, before, label, votes, margins):
    """the fixture holds what the issue asks the rooms to hold"""
    inst, sem, views = case["instance"].reshape(-1), case["semantic"].reshape(-1), case["views"]
    ids, counts = np.unique(inst, return_counts=True)
    seen_per = np.array([seen_any[inst == i].sum() for i in ids])
    assert 12 <= ids.size <= 30 and -1 in ids and (counts == 1).any() and (seen_per == 2).any() and (seen_per == 0).any()
    assert weak.sum() == ids.size and (sem[weak == 1] == -1).any()
    assert len(saved) == len(views) - 1 and out["visible"][-1] == 0 and views[-1]["key"] not in saved
    assert out["visible"][case["quiet"]] > 0 and out["prompts%d" % case["quiet"]].shape[0] == 0
    for v, view in enumerate(views[:-1]):  # visible, occluded (valid, in front, but hidden) and out-of-frame points
        assert 0 < out["visible"][v] < case["n"] // 2
    final = votes[-1]
    two = [p for p, s in final.items() if len(s) > 1]
    gained = lambda p, v: votes[v].get(p, set()) - (votes[v - 1].get(p, set()) if v else set())  # noqa: E731
    inside_one_view = sum(1 for p in two if any(len(gained(p, v)) > 1 for v in range(len(votes))))
    first = {p: min(v for v in range(len(votes)) if len(votes[v].get(p, ())) > 1) for p in two}
    across = sum(1 for p in two if first[p] > 0 and len(votes[first[p] - 1].get(p, ())) == 1)  # one class before that view
    own = sum(1 for p, s in final.items() if s == {int(sem[p])} and not weak[p])
    foreign_weak = sum(1 for p, s in final.items() if weak[p] and sem[p] != -1 and s != {int(sem[p])})
    print("  %s: %d instances, visible per view %s, prompts per view %s, %d labelled, %d dropped for two classes (%d inside one "
          "view, %d across views), %d weak points under a foreign mask, %d labels written over; margins %s"
          % (case["tag"], ids.size, out["visible"].tolist(), [out["prompts%d" % v].shape[0] for v in range(len(views))],
             (label != -1).sum(), len(two), inside_one_view, across, foreign_weak, (before != label).sum(),
             {k: "%.2e" % v for k, v in margins.items()}))
    assert inside_one_view > 0 and across > 0 and own > 20 and foreign_weak > 0 and (before != label).sum() > 0


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["POINTCEPT_ROOT"]
    code = load_ranges(ref)
    fx = {}
    for tag in PC.CASES:
        for k, v in run_case(code, tag).items():
            fx["%s_%s" % (tag, k)] = v
    path = os.path.join(HERE, "pp2s.npz")
    np.savez_compressed(path, **fx)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
