"""bench.py on one GPU at reduced sizes: a plain run prints the headline line only, --steps sets the number of
timed cycles, and --dump-outputs writes the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    n, steps = 64, 3
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _bench("--steps", steps, "--warmup", 1, "--n", n, "--dump-outputs", d)
        assert out["steps"] == steps and out["dtype"] == "f64" and out["unit"] == "LUP/s" and out["higher_is_better"]
        assert abs(out["value"] - 2 * 5 * n ** 3 / (out["ms_per_step"] * 1e-3)) < 1e-9 * out["value"]
        for k in ("roofline", "smoother", "solve", "configs", "end_to_end", "cpu_baseline"):
            assert k not in out, k                       # measured with --full only
        runs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sorted(runs[0]) == ["solve_returns.npy", "u.npy"]
    u, ret = runs[0]["u.npy"], runs[0]["solve_returns.npy"]
    assert u.shape == (n, n, n) and u.dtype == np.float64 and np.isfinite(u).all()
    assert ret[1] == steps and ret[2] > 0
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f


def test_dump_of_a_large_grid_is_a_sample(tmp_path):
    import bench
    n = 168                                              # 4.7 M points: more than bench.DUMP_POINTS
    _bench("--steps", 1, "--warmup", 0, "--n", n, "--dump-outputs", tmp_path)
    s = np.load(tmp_path / "u_sample.npy")
    assert s.shape == (bench.DUMP_POINTS,) and s.dtype == np.float64 and np.isfinite(s).all()
    idx = bench.dump_sample_index(n ** 3)
    # the sampled boundary points hold the Dirichlet data they were given (the solver leaves them alone)
    mesh, u0 = bench.boundary_problem(n)
    k, j, i = np.unravel_index(idx, (n, n, n))
    on_dirichlet_face = (j == 0) | (j == n - 1) | (k == 0) | (k == n - 1)
    assert on_dirichlet_face.any()
    assert np.array_equal(s[on_dirichlet_face], u0.ravel()[idx[on_dirichlet_face]])
