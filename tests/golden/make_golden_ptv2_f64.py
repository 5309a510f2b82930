"""Seed search for tests/ptv2_f64_cases.py (no fixture file is written: the cases are seeded, the seeds are recorded there).

    python -m tests.golden.make_golden_ptv2_f64 --seeds [--only NAME] [--candidates K]

For every Block case and mode and every model case: the first seed (of at most ptv2_f64_cases.SEARCH) for which, in the
float64 reference on the CPU, the smallest non-zero |ReLU pre-activation| and the smallest pooling gap are at least
HEADROOM * ptv2_ref64.RATIO times the largest |p32 - p64| (the eager float32 run's pre-activations against the float64 run's).  Forward
runs of the reference alone; tables from the oracle.  --candidates K prints the first K such seeds instead of one."""
import argparse
import sys

import torch

from oracle import pointops_ref as P
from tests import ptv2_f64_cases as C
from tests import ptv2_ref64 as R


# the search asks for a little more than the tests assert, so that a recorded seed survives a float32 run that rounds otherwise
HEADROOM = 1.1


def search(label, trial, want):
    found = []
    for seed in range(C.SEARCH):
        small, eps = trial(seed)
        if small >= HEADROOM * R.RATIO * eps:
            found.append((seed, small / eps))
            if len(found) == want:
                break
    if not found:
        print("%-28s NO SEED among %d meets the margin" % (label, C.SEARCH))
        return False
    print("%-28s %s" % (label, "  ".join("seed %d (ratio %.2f)" % f for f in found)), flush=True)
    return True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", action="store_true", required=True)
    ap.add_argument("--only", default=None)
    ap.add_argument("--candidates", type=int, default=1)
    args = ap.parse_args(argv)
    ok = True
    for name, case in C.BLOCK_CASES.items():
        if args.only and args.only != name:
            continue
        coord, offset = (torch.from_numpy(a) for a in C.block_cloud(name))
        idx = P.knn_query(case.k, coord, offset)[0]
        for mode in case.modes:
            ok &= search("block %s %s" % (name, mode), lambda s: C.block_reference(name, mode, s, coord, idx, grads=False)[2],
                         args.candidates)
    for name, case in C.MODEL_CASES.items():
        if args.only and args.only != name:
            continue
        coord, offset = (torch.from_numpy(a) for a in C.model_cloud(case.clouds))
        cfg = C.model_cfg(name)
        levels = R.oracle_tables(cfg, coord, offset)
        ok &= search("model %s" % name, lambda s: C.model_reference(cfg, case.training, s, coord, levels, grads=False)[2],
                     args.candidates)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
