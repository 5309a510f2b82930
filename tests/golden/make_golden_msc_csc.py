"""tests/golden/make_golden_msc_csc.py -- the MSC-v1m2 (CSC) fixtures, produced by CONSTRUCTING and RUNNING the reference's model
on the CPU under the stubs of make_golden_msc.py (imported, not changed):

    msc_csc_manifest.json   keys and shapes of the reference's MSC-v1m2 class over the default SpUNet-v1m1 backbone: "config"
                            (the ScanNet config's model: no heads, 3 input channels) and "heads" (the constructor's defaults)
    msc_csc_config.json     the `model` dict and both transform lists of configs/scannet/pretrain-msc-v1m2-0-spunet-csc.py, read
                            by running the config file: settings only
    msc_csc.npz             the batch of make_golden_msc.make_batch (two scenes, a few hundred points per view): the inputs, the
                            recorded backbone outputs, the state, the random tensors the reference drew, match_index, the output
                            of compute_partitions for every scene with a pair (`<prefix>part.<scene>`) and every entry of the
                            returned dict, for
                              a.*  r1 = 0.125, r2 = 0.5, matching_max_pair = MAX_PAIR_A, below the number of matches: the pairs
                                   interleave the scenes
                              b.*  the config's r1 = 2, r2 = 20 (larger than the rooms: every element is "none")
                            both with the config's mask_rate = 0, nce_t = 0.4 and no heads

Two margins are searched for and asserted: every kNN distance stays a relative MARGIN from the matching radius (the batch seed),
and every off-diagonal distance sqrt(|x_j - y_i|^2 + 1e-7) of a scene's pairs, in float64, stays a relative MARGIN from r1 and
from r2 (the seed of the draws of a.*): the class of an element inside that margin is not pinned.  MAX_PAIR_A is small because
of the second: at a few hundred pairs per scene some element always falls inside it.

usage:  python tests/golden/make_golden_msc_csc.py <reference root>
"""
import json
import os
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_msc as MM  # noqa: E402
from tests import msc_csc_ref as C  # noqa: E402

MARGIN = MM.MARGIN
MAX_PAIR_A = 64
CONFIG = "pretrain-msc-v1m2-0-spunet-csc.py"
COMMON = dict(mask_grid_size=0.1, mask_rate=0, nce_t=0.4, reconstruct_color=False, reconstruct_normal=False, partitions=4)


def record_config(ref):
    cfg = runpy.run_path(os.path.join(ref, "configs", "scannet", CONFIG))
    out = dict(config="configs/scannet/" + CONFIG, model=cfg["model"],
               **{k: v for k, v in cfg["data"]["train"].items() if k.endswith("transform")})
    path = os.path.join(HERE, "msc_csc_config.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("msc_csc_config.json", os.path.getsize(path), "bytes,", sorted(out))
    return out


def radius_margin(batch, pairs, r1, r2):
    """the smallest relative distance of an off-diagonal d from r1 or r2 over the scenes, and the classes seen"""
    scene = C.scenes_of(pairs, batch["view1_offset"], len(batch["view1_origin_coord"]))
    worst, seen = np.inf, set()
    for s in np.unique(scene):
        rows = np.nonzero(scene == s)[0]
        x, y = batch["view1_origin_coord"][pairs[rows, 0]], batch["view2_origin_coord"][pairs[rows, 1]]
        d = C.distances64(x, y)
        off = ~np.eye(len(rows), dtype=bool)
        if off.any():
            worst = min(worst, float(np.abs(d[off] - r1).min() / r1), float(np.abs(d[off] - r2).min() / r2))
        seen |= set(C.classes(x, y, r1, r2).numpy()[off].tolist())
    return worst, seen


def record(cls, batch, out, prefix, seed, **cfg):
    parts = []
    inner = cls.compute_partitions
    cls.compute_partitions = lambda self, c1, c2: parts.append(inner(self, c1, c2)) or parts[-1]
    try:
        res = MM.record_model(cls, batch, out, prefix, seed, **dict(COMMON, **cfg))
    finally:
        cls.compute_partitions = inner
    pairs = out[prefix + "match_index"]
    scenes = np.unique(C.scenes_of(pairs, batch["view1_offset"], len(batch["view1_origin_coord"])))
    assert len(parts) == len(scenes)
    for s, part in zip(scenes, parts):
        out[prefix + "part.%d" % s] = part.numpy()
    return res


def main():
    ref = sys.argv[1]
    config = record_config(ref)
    models = MM.load_reference(ref)
    MM._load("pointcept.models.masked_scene_contrast.masked_scene_contrast_v1m2_csc",
             os.path.join(ref, "pointcept", "models", "masked_scene_contrast", "masked_scene_contrast_v1m2_csc.py"))
    cls = models["MSC-v1m2"]
    manifest = {}
    for name, kwargs in (("config", {k: v for k, v in config["model"].items() if k != "type"}),
                         ("heads", dict(backbone=dict(config["model"]["backbone"], in_channels=6), backbone_in_channels=6,
                                        backbone_out_channels=96))):
        manifest[name] = {k: list(v.shape) for k, v in cls(**kwargs).state_dict().items()}
    path = os.path.join(HERE, "msc_csc_manifest.json")
    with open(path, "w") as f:  # compact, one key per line
        f.write("{\n%s\n}\n" % ",\n".join(' %s: {\n%s\n }' % (json.dumps(name), ",\n".join(
            "  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in keys.items())) for name, keys in manifest.items()))
    print("msc_csc_manifest.json", os.path.getsize(path), "bytes,", {k: len(v) for k, v in manifest.items()}, "keys")

    for seed in range(MM.SEED, MM.SEED + 100):  # the first seed whose kNN distances keep the margin
        batch = MM.make_batch(seed)
        margin, matched = MM.margin_of(batch)
        if margin > MARGIN:
            break
    assert margin > MARGIN, "no seed keeps the kNN margin"
    assert matched > MAX_PAIR_A
    for draw_seed in range(seed + 1, seed + 201):  # the first draws whose pairs keep the margin from r1 and r2
        out = dict(batch, seed=np.array(seed, np.int64), radius=np.array(MM.RADIUS), max_k=np.array(MM.MAX_K, np.int64))
        a = record(cls, batch, out, "a.", draw_seed, matching_max_pair=MAX_PAIR_A, r1=0.125, r2=0.5)
        d_margin, seen = radius_margin(batch, out["a.match_index"], 0.125, 0.5)
        if d_margin > MARGIN and seen == {0, 1, 2, 3, C.NONE}:
            break
    assert d_margin > MARGIN and seen == {0, 1, 2, 3, C.NONE}, "no draw keeps the margin from r1 and r2 with every class present"
    b = record(cls, batch, out, "b.", draw_seed + 1000, matching_max_pair=8192, r1=2, r2=20)
    b_margin, b_seen = radius_margin(batch, out["b.match_index"], 2.0, 20.0)
    assert b_margin > MARGIN and b_seen == {C.NONE}
    out["a.max_pair"], out["a.r"], out["b.r"] = np.array(MAX_PAIR_A, np.int64), np.array([0.125, 0.5]), np.array([2.0, 20.0])
    out["draw_seed"] = np.array(draw_seed, np.int64)
    assert len(out["a.match_index"]) == MAX_PAIR_A and len(out["a.pair_perm"]) == matched and len(out["b.match_index"]) == matched
    scene_a = C.scenes_of(out["a.match_index"], batch["view1_offset"], len(batch["view1_origin_coord"]))
    assert (np.diff(scene_a) < 0).any(), "the pairs of a.* interleave the scenes"
    path = os.path.join(HERE, "msc_csc.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "msc.npz"))
    print("msc_csc.npz", os.path.getsize(path), "bytes, seed", seed, "draw seed", draw_seed, ", kNN margin %.2e, radius margin %.2e (a) "
          "%.2e (b)," % (margin, d_margin, b_margin), matched, "matched rows,", {k: float(v) for k, v in a.items()},
          {k: float(v) for k, v in b.items()})


if __name__ == "__main__":
    main()
