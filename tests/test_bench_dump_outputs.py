"""bench.py --dump-outputs DIR: the crowd the headline leg's last timed step computed, as DIR/<field>.npy.

CPU tests: the writer (float64, ascending id, a fixed seeded sample above the size cap) and the argument guard.
GPU test: two runs with the same arguments write the same arrays, bit for bit, and --steps sets the timed steps.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module("bench")


def _crowd(n):
    from rmf_crowdsim_amd.simulation import AGENT_DTYPE
    c = np.zeros(n, dtype=AGENT_DTYPE)
    c["id"] = np.arange(n) + 1
    rng = np.random.default_rng(3)
    for f in ("x", "y", "vx", "vy"):
        c[f] = rng.standard_normal(n)
    c["next_waypoint"] = np.arange(n) % 3
    return c


def test_dump_writes_every_field_as_float64(tmp_path):
    bench = _bench()
    c = _crowd(1000)
    bench.dump_outputs(str(tmp_path / "out"), c)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f + ".npy" for f in bench.DUMP_FIELDS)
    for f in bench.DUMP_FIELDS:
        a = np.load(tmp_path / "out" / (f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (1000,)
        assert np.array_equal(a, c[f].astype(np.float64))


def test_dump_above_the_cap_is_the_same_seeded_sample_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 48 * 300)
    c = _crowd(1000)
    bench.dump_outputs(str(tmp_path / "a"), c)
    bench.dump_outputs(str(tmp_path / "b"), c)
    total = 0
    for f in bench.DUMP_FIELDS:
        a, b = np.load(tmp_path / "a" / (f + ".npy")), np.load(tmp_path / "b" / (f + ".npy"))
        assert a.shape == (300,) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 48 * 300
    ids = np.load(tmp_path / "a" / "id.npy")
    assert (np.diff(ids) > 0).all()
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), c["x"][ids.astype(np.int64) - 1])


def test_dump_outputs_with_the_python_mesh_is_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--mesh", "python", "--dump-outputs", "unused"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--mesh native" in p.stderr


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--agents", "20000", "--steps", "7", "--warmup", "2",
                            "--clock-warmup", "3", "--no-cpu-baseline", "--no-creep-leg",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 7
        dumps.append({f: np.load(tmp_path / run / (f + ".npy")) for f in ("id", "x", "y", "vx", "vy", "next_waypoint")})
    a, b = dumps
    assert a["id"].shape == (20000,) and (np.diff(a["id"]) > 0).all()
    assert np.isfinite(a["x"]).all() and np.isfinite(a["vx"]).all()
    for f in a:
        assert a[f].dtype == np.float64
        assert np.array_equal(a[f], b[f]), f
