"""bench.py's launch contract (CPU): a multi-GPU request is either a torchrun world of
that size or a torchrun child launch; a single process never reports N GPUs."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_mismatched_world_size_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr
    assert "{" not in r.stdout  # no bench line


def test_gpus_without_torchrun_relaunches_n_ranks(monkeypatch):
    seen = {}

    def fake_run(cmd, *a, **kw):
        seen["cmd"] = cmd

        class R:
            returncode = 0
        return R()
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "7", "--warmup", "2"])
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "127.0.0.1" in cmd
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "7", "--warmup", "2"]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def _fake_outputs(T, S, W):
    import torch
    g = torch.Generator().manual_seed(3)
    return {"traj": torch.rand((T, S, W), dtype=torch.float64, generator=g),
            "chi": torch.rand(W, dtype=torch.float64, generator=g),
            "ssres": torch.rand(W, dtype=torch.float64, generator=g),
            "status": torch.arange(W, dtype=torch.int32) % 3}


def test_dump_outputs_writes_every_array_whole_when_it_fits(tmp_path):
    import numpy as np
    out = _fake_outputs(7, 3, 50)
    shapes = bench.dump_outputs(str(tmp_path / "d"), out)
    assert shapes == {"traj": [7, 3, 50], "walkers": [50], "chi": [50], "ssres": [50], "status": [50]}
    for name in shapes:
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float64 and list(a.shape) == shapes[name]
    assert np.array_equal(np.load(tmp_path / "d" / "traj.npy"), out["traj"].numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "status.npy"), out["status"].numpy().astype(float))
    assert np.array_equal(np.load(tmp_path / "d" / "walkers.npy"), np.arange(50.0))


def test_dump_outputs_samples_the_same_walkers_every_run(tmp_path, monkeypatch):
    """A trajectory larger than the budget is sampled: distinct sorted walkers, the same in
    every run, the sampled columns unchanged; beyond DUMP_FULL_WALKERS the per-walker
    vectors hold the same walkers."""
    import numpy as np
    T, S, W = 5, 2, 300
    monkeypatch.setattr(bench, "DUMP_TRAJ_BYTES", T * S * 8 * 40)
    monkeypatch.setattr(bench, "DUMP_FULL_WALKERS", 100)
    out = _fake_outputs(T, S, W)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
        runs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("traj", "walkers", "chi", "ssres", "status")})
    for n in runs[0]:
        assert np.array_equal(runs[0][n], runs[1][n])
    idx = runs[0]["walkers"].astype(int)
    assert len(idx) == 40 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < W
    assert np.array_equal(runs[0]["traj"], out["traj"].numpy()[:, :, idx])
    assert np.array_equal(runs[0]["chi"], out["chi"].numpy()[idx])
    assert sum(a.nbytes for a in runs[0].values()) <= T * S * 8 * 40 + 4 * 8 * 40


def test_host_cores_reports_the_affinity_set():
    cores, detail = bench.host_cores()
    assert 1 <= cores <= len(os.sched_getaffinity(0))
    assert detail["sched_getaffinity"] == len(os.sched_getaffinity(0))
