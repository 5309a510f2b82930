"""tests/msc_cases.py -- what the Masked Scene Contrast tests share: the fixtures of tests/golden (make_golden_msc.py), helpers on
them, and the tolerances of the M-rule with the ratios they come from."""
import json
import os

import numpy as np

from tests import msc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 2.0 ** -24

# e_kernel <= M_TOL * max(e_eager, FLOOR) against float64; M_TOL = twice the worst ratio measured on an MI355X, rounded up to a
# power of two, at least 1 and at most 64
# (worst ratios: loss 5.24 at M = 65, t = 0.07; pos_sim 1.36; neg_sim 1.07; df1 3.39 and df2 3.18 at M = 2)
M_TOL = dict(loss=16, pos_sim=4, neg_sim=4, df1=8, df2=8)
# the running-max form of the row logsumexp (t < 0.025), at t = 0.02: gradients 11.7 times the eager error, the loss 41.4 times
# (twice that is past the rule's ceiling of 64, which therefore is the bound): lse - pos / t is formed from two numbers of
# magnitude 1 / t = 50, where the eager log-softmax subtracts the row maximum first
M_TOL_RUNNING_MAX = dict(M_TOL, loss=64, df1=32, df2=32)
# the reconstruction losses are eager on both sides; against the recorded CPU run their error is 0.67 times its own at the worst
M_TOL_EAGER = 2
# HIP against AO_AMD_MSC=torch over a small real SpUNetBase (tests/test_gpu_msc_model.py): the distance between the paths over
# 2^-24 of the eager value (returned entries) or of the eager gradient's norm (relative L2, the worst parameter)
# (measured: pos_sim 2.04, the other entries below 0.01; the worst gradient 20.65, the median 11.3)
M_TOL_PATHS = dict(nce_loss=1, pos_sim=8, neg_sim=1, color_loss=1, normal_loss=1, loss=1, grad=64)
# the mean of the gray values in RandomColorJitter's contrast: 0.50 times the error of numpy's mean
M_TOL_MEAN = 1


def fixture():
    with np.load(os.path.join(GOLDEN, "msc.npz")) as f:
        return {k: f[k] for k in f.files}


def configs():
    """{"base": dict(model, transform), "pointcontrast": dict(model, view1_transform, view2_transform)}: the settings of the
    reference's two MSC-v1m1 ScanNet configs as recorded data"""
    with open(os.path.join(GOLDEN, "msc_configs.json")) as f:
        return json.load(f)


def model_kwargs(cfg):
    return {k: v for k, v in cfg["model"].items() if k != "type"}


def knn_of(fix):
    return R.knn_bruteforce(int(fix["max_k"]), fix["view2_origin_coord"], fix["view2_offset"], fix["view1_origin_coord"],
                            fix["view1_offset"])


def heads64(fix, prefix, name, feat, mask):
    w, b = fix[prefix + "state.%s.weight" % name].astype(np.float64), fix[prefix + "state.%s.bias" % name].astype(np.float64)
    return feat[mask].astype(np.float64) @ w.T + b
