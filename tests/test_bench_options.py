"""bench.py's command line without a GPU: a plain run keeps only the headline's own timed region (every leg that takes runs of
its own waits for --full), and --dump-outputs writes float32 arrays within a size cap, the same sample for the same shape."""
import importlib.util
import os
import sys

import numpy as np

from tests.conftest import ROOT

LEGS = ("no_cpu_baseline", "no_roofline", "no_ops", "no_reference_loop", "no_also")


def _bench(monkeypatch):
    # (bench.py sets an environment default and prepends its directory to sys.path at import: both are undone after the test)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    monkeypatch.setattr(sys, "path", list(sys.path))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(monkeypatch, mod, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return mod.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    mod = _bench(monkeypatch)
    args = _parse(monkeypatch, mod, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not args.full and args.steps == 7 and args.warmup == 2 and args.dump_outputs is None
    assert all(getattr(args, k) for k in LEGS)


def test_full_runs_every_leg_unless_switched_off(monkeypatch):
    mod = _bench(monkeypatch)
    args = _parse(monkeypatch, mod, "--full")
    assert args.full and not any(getattr(args, k) for k in LEGS)
    args = _parse(monkeypatch, mod, "--full", "--no-ops", "--no-also", "--dump-outputs", "out")
    assert args.no_ops and args.no_also and not args.no_roofline and not args.no_reference_loop and not args.no_cpu_baseline
    assert args.dump_outputs == "out"


def test_dump_outputs_writes_float32_within_the_cap(monkeypatch, tmp_path):
    mod = _bench(monkeypatch)
    mod._imports()
    monkeypatch.setattr(mod, "DUMP_CAP", 1300)
    rng = np.random.default_rng(7)
    big = rng.standard_normal((1000, 13))
    flat = rng.standard_normal(5000).astype(np.float32)
    small = mod.torch.arange(6, dtype=mod.torch.int64).reshape(2, 3)
    got = mod.dump_outputs(str(tmp_path / "a"), {"big": big, "flat": flat, "small": small, "loss": np.float64(0.5)})
    assert got["big"] == ([100, 13], [1000, 13]) and got["flat"] == ([1300], [5000]) and got["small"] == ([2, 3], [2, 3])
    files = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("big", "flat", "small", "loss")}
    assert all(a.dtype == np.float32 for a in files.values())
    assert np.array_equal(files["small"], np.arange(6, dtype=np.float32).reshape(2, 3)) and files["loss"] == np.float32(0.5)
    # the sample is whole rows of the array, in their order, and the same rows on every call
    rows = [int(np.flatnonzero((big.astype(np.float32) == r).all(axis=1))[0]) for r in files["big"]]
    assert rows == sorted(set(rows)) and len(rows) == 100
    assert set(files["flat"].tolist()) <= set(flat.tolist())
    mod.dump_outputs(str(tmp_path / "b"), {"big": big * 2})
    assert np.array_equal(np.load(str(tmp_path / "b" / "big.npy")), 2 * files["big"])
