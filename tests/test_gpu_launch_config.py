"""GPU: the dynamic-LDS limit of a kernel that is launched with shape-dependent sizes (ao_amd/csrc/abi.hip: ptv2_kernel_lds).

hipFuncSetAttribute(MaxDynamicSharedMemorySize) SETS the limit of a kernel on the current device.  ptv2_kernel_lds keeps the
largest value it has set per (kernel, device) and calls the runtime only for a larger one, so the ORDER in which a process first
uses the shapes of one kernel is what is under test: narrow, wide, narrow (the limit must go up for the wide launch and must not
come down before the third) and wide, narrow, wide.  Every scenario therefore runs in a child process of its own, started with
`python -m tests.test_gpu_launch_config <scenario> <order>`, and every launch in it is held to the float64 reference and bound of
the suite that owns the launcher -- no tolerance is introduced here:

  skinny   tests/test_gpu_dense_f64.py::skinny_check (tests/dense_ref64.py::skinny, the M table there) at n = 257 for
           (cin, cout) = (48, 6), a few KB of LDS, and (384, 48): at least 48 x 388 floats = 74 KB in the tile form, 78 KB in the
           lane form (AO_AMD_SKINNY=lanes, read per call) -- both above the 64 KB a kernel may use without asking
  peb      gva_peb_forward_hip_launcher on peb_fwd_kernel (c / g != 8): c = 512, g = 32 stages 32 x 516 floats = 66 KB, c = 48,
           g = 12 stages 10 KB; n = 1, the smallest n of tests/test_gpu_gva_f64.py's staged form.  A, sw and out_v are the eager
           fp32 statement's own (tests/gva_ref64.py::statement: the aggregate launcher has no instance for these group counts),
           `out` is held to gva_ref64.project in float64 on those operands with M["out"] of tests/test_gpu_gva_f64.py against
           the eager fp32 projection of the same operands
  devices  the wide skinny case on device 0, then on device 1: the table is per device (skipped with one device visible)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERS = dict(narrow_first=("narrow", "wide", "narrow"), wide_first=("wide", "narrow", "wide"))
SKINNY = dict(narrow=(257, 48, 6), wide=(257, 384, 48))
PEB = dict(narrow=(1, 48, 12), wide=(1, 512, 32))


# ------------------------------------------------------------------------------------------------------------------ the children
def _skinny(which):
    from tests import dense_ref64 as R
    from tests import test_gpu_dense_f64 as D

    n, cin, cout = SKINNY[which]
    D.skinny_check(R.SkinnyCase("skinny-n%d-%dto%d" % (n, cin, cout), n, cin, cout))


def _peb(which):
    import torch

    from ao_amd import _lib
    from tests import gva_ref64 as R
    from tests import test_gpu_gva_f64 as G

    n, c, g = PEB[which]
    case = R.Case("std-n%d-c%d-g%d-k16" % (n, c, g), n, c, g, 16, "std")
    t = R.build_inputs(case, G._gpu_knn, device="cuda")
    ops = {key: val.contiguous() for key, val in R.statement(t, torch.float32, backward=False).items() if key in ("A", "sw", "out_v")}
    out = G._nan(n, c)
    _lib.check(_lib.lib().gva_peb_forward_hip_launcher(n, c, g, ops["A"].data_ptr(), *G._p(t, "Wp2", "bp2"), *G._p(ops, "sw", "out_v"),
                                                      out.data_ptr(), _lib.stream_ptr()), "gva_peb_forward_hip_launcher")
    torch.cuda.synchronize()
    project = lambda dt: R.project(ops["A"].to(dt), t["Wp2"].to(dt), t["bp2"].to(dt), ops["sw"].to(dt), ops["out_v"].to(dt))
    ref = project(torch.float64)
    (ek, mk), (ee, me) = R.errors(out, ref), R.errors(project(torch.float32), ref)
    print("f64 %s peb out e_kernel %.3e e_eager %.3e ratio %.2f | max %.3e %.3e ratio %.2f" % (
        case.name, ek, ee, ek / max(ee, 1e-300), mk, me, mk / max(me, 1e-300)))
    assert bool(torch.isfinite(out).all()), (case.name, "not finite (an unwritten row shows as NaN)")
    assert ek <= G.M["out"] * ee, (case.name, "relative L2", ek, ee, G.M["out"])
    assert mk <= G.M["out"] * me, (case.name, "largest element", mk, me, G.M["out"])


def _devices():
    import torch

    from tests import test_gpu_dense_f64 as D

    for device in (0, 1):
        torch.cuda.set_device(device)
        D._CACHE.clear()  # (the cached operands live on the device they were made on)
        _skinny("wide")
        print("device %d done" % device)


def child(scenario, order):
    if scenario == "devices":
        return _devices()
    for which in ORDERS[order]:
        dict(skinny=_skinny, peb=_peb)[scenario](which)
        print("%s %s done" % (scenario, which))


# --------------------------------------------------------------------------------------------------------------------- the tests
def _run(scenario, order, lanes=False):
    env = {key: val for key, val in os.environ.items() if key != "AO_AMD_SKINNY"}
    if lanes:
        env["AO_AMD_SKINNY"] = "lanes"
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_launch_config", scenario, order], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("form", ["tiles", "lanes"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_skinny_limit_follows_the_widest_shape_whatever_came_first(order, form):
    out = _run("skinny", order, lanes=form == "lanes")
    assert [line.split()[1] for line in out.splitlines() if line.startswith("skinny ") and line.endswith(" done")] == list(ORDERS[order])


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_peb_limit_follows_the_widest_shape_whatever_came_first(order):
    out = _run("peb", order)
    assert [line.split()[1] for line in out.splitlines() if line.startswith("peb ") and line.endswith(" done")] == list(ORDERS[order])


def test_limit_is_kept_per_device():
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: the second device's first launch cannot be exercised")
    out = _run("devices", "-")
    assert "device 0 done" in out and "device 1 done" in out


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
