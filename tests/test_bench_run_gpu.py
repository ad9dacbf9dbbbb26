"""bench.py as the driver runs it, on the GPU: a plain run times the headline's steps and nothing else, and --dump-outputs writes
the state its last timed step left -- the same files, bit for bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    names = ("walkers", "X", "lnL", "lp", "nacc", "nswap", "cov")
    runs = []
    for tag in ("a", "b"):
        out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / tag))
        assert out["steps"] == 3 and out["warmup"] == 1 and out["iterations_timed"] == 300
        assert out["unit"] == "updates/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert out["value"] > 0 and out["ms_per_step"] > 0
        assert "also" not in out and "cpu_baseline" not in out and out["ess_per_sec"] is None       # the rest is --full's
        files = sorted(os.listdir(str(tmp_path / tag)))
        assert files == sorted(n + ".npy" for n in names)
        assert sum(os.path.getsize(str(tmp_path / tag / f)) for f in files) <= 64 * 10 ** 6
        runs.append({n: np.load(str(tmp_path / tag / (n + ".npy"))) for n in names})
    a, b = runs
    nw = len(a["walkers"])
    assert 1 <= nw <= 4096 and a["X"].shape == (nw, 64, 100) and a["lnL"].shape == (nw, 64) and a["cov"].shape == (1, 100, 100)
    assert all(a[n].dtype == np.float64 for n in names)
    assert np.all(np.isfinite(a["X"])) and np.any(a["X"] != 0) and np.all(a["nacc"] > 0)      # the chains moved
    for n in names:
        assert np.array_equal(a[n].view(np.uint64), b[n].view(np.uint64)), n
