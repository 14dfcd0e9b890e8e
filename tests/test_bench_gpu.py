"""A plain bench.py run on the GPU (a small LQR batch): the result line's headline
fields, nothing measured beyond the timed steps, and the --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dump(tmp_path):
    from crocoddyl_amd import synthetic
    from crocoddyl_amd.dist import RESULT_FIELDS
    cfg, B, steps = "C2_lqr", 4, 2
    _, n, m, T, _, _ = synthetic.CONFIGS[cfg]
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--config", cfg, "--batch", str(B), "--dump-outputs", out],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["unit"] == "FDDP iterations/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    assert r["steps"] == steps and r["ms_per_step"] > 0 and r["value"] > 0
    # value and ms_per_step are the same measurement: iterations of the timed steps / their time
    iters = sum(r["ranks"]["iterations"])
    assert 0 < iters <= B * steps
    assert r["value"] == pytest.approx(iters / (r["ms_per_step"] * steps * 1e-3), rel=1e-3)
    # what takes runs of its own is behind --full
    assert r["cpu_baseline"] is None and r["secondary_protocol"] is None and "speedup_vs_cpu" not in r
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ["elements", "results", "us", "xs"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["elements"], np.arange(B))
    assert got["xs"].shape == (B, T + 1, n) and got["us"].shape == (B, T, m)
    assert got["results"].shape == (B, len(RESULT_FIELDS))
    assert all(np.isfinite(a).all() for a in got.values())
    # the dump is one step's solve, solve(maxiter=1): at most one iteration run per element
    assert set(np.unique(got["results"][:, RESULT_FIELDS.index("n_iter_run")])) <= {0.0, 1.0}
