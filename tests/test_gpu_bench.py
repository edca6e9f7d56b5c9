"""bench.py's plain run on the device: the headline only, and ``--dump-outputs``.

One small plain run (4 096 walkers, 200 output times, 3 timed steps) as a child process:
the line carries the headline fields and none of the ``--full`` legs, and the dumped arrays
are what the timed ``integrate`` returned — RK4 trajectories bitwise equal to the C
restatement (oracle/rk_ref.c) of the same seeded inputs, chi within rtol 1e-11 (the bar
``__graft_entry__.smoke`` holds the same kernel to).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import rk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

W, T, STEPS = 4096, 200, 3


def test_plain_run_reports_the_headline_only_and_dumps_its_outputs(tmp_path):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--warmup-ms", "5", "--walkers", str(W), "--times", str(T),
                        "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == STEPS and line["n_gpus"] == 1 and line["dtype"] == "f64" and line["higher_is_better"]
    assert line["unit"] == "walker-timesteps/s" and line["ms_per_step"] > 0 and line["chi_finite"]
    assert line["value"] == pytest.approx(W * (T - 1) / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert line["full"] is False
    assert line["cpu_baseline"] is None and line["mcmc"] is None and line["other_configs"] is None
    assert line["roofline"]["traffic"] is None and line["roofline"]["box_write_ceiling"] is None
    assert line["dumped_outputs"]["traj"] == [T, 4, W]

    got = {n: np.load(d / f"{n}.npy") for n in ("traj", "walkers", "chi", "ssres", "status")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["walkers"], np.arange(W))
    m, y0h = bench.build_problem("two_i", "rk4", T)
    theta = np.ascontiguousarray(bench.synthetic_walkers(W, 5))
    y0 = np.ascontiguousarray(np.repeat(y0h[:, None], W, axis=1))
    ref = rk_ref.integrate(m.fit_problem(), y0, theta, trajectory=True)
    assert np.array_equal(got["traj"], ref["traj"])
    np.testing.assert_allclose(got["chi"], ref["chi"], rtol=1e-11)
    assert not got["status"].any()
