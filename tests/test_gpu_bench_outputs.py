"""`bench.py --dump-outputs DIR` end to end on one MI355X: a plain run times exactly --steps steps, its line carries the
headline fields and none of the --full legs, and the arrays of its last timed step land in DIR as float32; a second run with
the same arguments starts from the same inputs and ends at the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

POINTS = 20000


def _bench(out_dir):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--points", str(POINTS), "--dump-outputs", out_dir], env=e, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy"))
                                  for n in ("loss", "logits", "params", "grads", "buffers")}


def test_plain_run_dumps_its_last_step(tmp_path):
    line, out = _bench(str(tmp_path / "a"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and len(line["host"]["step_ms"]["in_order"]) == 3 and line["dtype"] == "fp32"
    assert not {"roofline", "reference_loop", "ops", "cpu_baseline"} & set(line) and "also" not in line["config"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert out["loss"].shape == (1,) and out["loss"][0] == np.float32(line["config"]["loss"])
    n = line["config"]["points_per_gpu"]
    assert out["logits"].shape == (n, 13) and out["params"].shape == out["grads"].shape == (3908641,)
    assert np.abs(out["grads"]).max() > 0 and out["buffers"].size > 0
    again, out2 = _bench(str(tmp_path / "b"))
    assert again["config"]["points_per_gpu"] == n
    for name, a in out.items():
        np.testing.assert_allclose(out2[name], a, rtol=1e-4, atol=1e-5, err_msg=name)
