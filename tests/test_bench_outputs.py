"""bench.py --steps / --dump-outputs: the timed region is exactly K steps, and what its last step returned is written
as float32 / float64 .npy files that a second run with the same arguments reproduces to the last bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(directory):
    return {name[:-4]: np.load(os.path.join(directory, name)) for name in sorted(os.listdir(directory))}


def test_steps_default_is_the_workloads_and_an_explicit_count_is_kept():
    for name, spec in bench.WORKLOADS.items():
        assert bench.parse_args(["--workload", name]).steps == spec["steps"] > 0
        assert bench.parse_args(["--workload", name, "--steps", "7"]).steps == 7


def test_dump_outputs_writes_float_arrays(tmp_path):
    arrays = {"actions": np.arange(5, dtype=np.int32), "visits": np.arange(10, dtype=np.int32).reshape(5, 2),
              "root_predicted": np.linspace(0, 1, 5, dtype=np.float32), "depth_sum": np.full(5, 2 ** 40, np.int64)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = _load(tmp_path / "out")
    assert sorted(got) == sorted(arrays)
    for name, a in arrays.items():
        assert got[name].dtype == (np.float32 if a.dtype == np.float32 else np.float64)
        assert np.array_equal(got[name], a)


def test_dump_outputs_over_the_limit_keeps_a_fixed_sample_of_envs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    arrays = {"actions": np.arange(4096, dtype=np.int32), "visits": np.arange(4096 * 9, dtype=np.int32).reshape(4096, 9)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    keep = a["env_index"].astype(np.int64)
    assert 0 < len(keep) < 4096 and (np.diff(keep) > 0).all()
    assert np.array_equal(a["actions"], arrays["actions"][keep]) and np.array_equal(a["visits"], arrays["visits"][keep])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 10


@pytest.mark.gpu
@pytest.mark.parametrize("workload,envs", [("cartpole", 4096), ("tictactoe", 4096)])
def test_bench_times_k_steps_and_reproduces_its_dump(tmp_path, workload, envs):
    runs = []
    for run in ("a", "b"):
        proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload,
                               "--envs", str(envs), "--steps", "7", "--warmup", "2", "--cpu-seconds", "0",
                               "--profile-steps", "0", "--dump-outputs", str(tmp_path / run)],
                              cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr[-2000:]
        runs.append((json.loads([line for line in proc.stdout.splitlines() if line.startswith("{")][0]),
                     _load(tmp_path / run)))
    (line, a), (_, b) = runs
    assert line["steps"] == line["timed_steps"] == 7 and line["moves_scheduled"] == 7 * envs
    assert abs(line["ms_per_step"] * 7 - 1e3 * line["timed_seconds"]) < 1e-6
    assert sorted(a) == sorted(b) and {"actions", "visits", "root_value_sum"} <= set(a)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and len(a[name]) == envs
        assert np.array_equal(a[name], b[name]), f"{name} differs between two runs with the same arguments"
    # a finished search: every simulation is a visit of one root child, and the action is one of the visited children
    # (statistics are per child slot; with every action legal, as in CartPole, slot == action)
    played = a["actions"] >= 0
    assert played.mean() > 0.99
    assert (a["visits"][played].sum(axis=1) == line["config"]["simulations"]).all()
    slots = a.get("action_slots", a["actions"])[played].astype(np.int64)
    assert (a["visits"][played, slots] > 0).all()
