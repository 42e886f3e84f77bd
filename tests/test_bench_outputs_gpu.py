"""bench.py's plain run and `--dump-outputs` (GPU): one small C1 run in a
child process.  The plain line carries the headline keys only, `--steps` is
the number of timed steps, and the dumped arrays are the last timed step's
outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "phase_ms_per_step", "timeline_ms_per_eval", "pair_kernels_tflops",
             "pair_kernels_hbm_gbs", "predict", "r6_drop_in", "cpu_baseline", "sharded")


@pytest.mark.timeout(120)
def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "C1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    # value = steps / (steps * ms_per_step): the two describe the same interval
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 1.0) < 1e-9
    assert not [k for k in FULL_ONLY if k in d]

    assert sorted(os.listdir(out)) == ["gradients.npy", "parameters.npy", "stats.npy"]
    a = {k: np.load(out / (k + ".npy")) for k in ("gradients", "parameters", "stats")}
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in a.values())
    assert a["stats"].shape == (2,) and a["gradients"].shape == a["parameters"].shape
    assert a["gradients"].size > 2 and np.any(a["gradients"] != 0.0)
    # the dumped statistics are the ones of the last timed step (the line's)
    assert a["stats"].tolist() == d["last_stats"]
