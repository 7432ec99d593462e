"""csrc/replay_sampler.h -- the arithmetic of the replay store's device sampler (ReplayBuffer.get_batch's draws and
update_priorities, include/mzreplay.h mzreplay_sample_batch / mzreplay_update_priorities) -- built for the host with g++
(tests/replay_sampler_check.cpp) and held to numpy and to the reference's recorded batches:

* the restated pairwise float32 sum against numpy.sum, bit for bit;
* one whole batch from numpy.random.seed(seed) against index_batch / weight_batch of the four G12 fixtures, and the
  stream left where numpy's own RandomState stands after the same draws;
* update_priorities against a plain sequential numpy loop (batch order, rows clipped, evicted ids skipped, game maximum);
* the C ABI of the feature: declared, exported, bound; refused without the sampler switched on.

The device build of the same header is checked on the GPU by tests/test_gpu_replay_sampler.py."""
import importlib
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from parity_helpers import load_golden
from test_oracle_replay import NAMES, cfg_of, games_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    work = tmp_path_factory.mktemp("replay_sampler")
    exe = str(work / "replay_sampler_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "replay_sampler_check.cpp")], check=True)

    def run(mode, payload):
        path = str(work / f"{mode}.bin")
        with open(path, "wb") as f:
            f.write(payload)
        proc = subprocess.run([exe, mode, path], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        return json.loads(proc.stdout.strip().splitlines()[-1])
    return run


def f32_of_bits(values):
    return np.array(values, dtype=np.uint32).view(np.float32)


def test_pairwise_sum_equals_numpy_sum(check):
    rs = np.random.RandomState(5)
    arrays = []
    for n in list(range(1, 301)) + [1000, 4096, 8191, 8192, 8200, 9999, 10000, 20001,
              65032, 65033, 65040, 65536, 65537, 70001, 140001]:
        for kind in range(3):
            exponents = rs.uniform(-12, 3, size=n) if kind < 2 else rs.uniform(-1, 0, size=n)
            a = (10.0 ** exponents).astype(np.float32)
            if kind == 1:
                a[rs.random_sample(n) < 0.3] = 0
            if kind == 2:
                a = np.sqrt(a)                                  # narrow range: every addition rounds
            arrays.append(a)
    payload = struct.pack("<i", len(arrays)) + b"".join(struct.pack("<i", len(a)) + a.tobytes() for a in arrays)
    got = f32_of_bits(check("sum", payload)["sums"])
    want = np.array([np.sum(a) for a in arrays], dtype=np.float32)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the sum is not the left-to-right one: the check above means something
    assert any(np.float32(sum(a.tolist())) != np.sum(a) for a in arrays if len(a) > 200)


class NumpyRng:
    """oracle.replay_oracle.get_batch's generator interface over numpy's own legacy RandomState."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def choice_p(self, p):
        return int(self.rs.choice(len(p), p=p))

    def below(self, n):
        return int(self.rs.choice(n))


def batch_payload(fx, cfg, priorities, game_priority):
    G, stride = priorities.shape
    head = struct.pack("<iiiiiiIq", G, stride, cfg["num_unroll_steps"], len(cfg["action_space"]), int(cfg["PER"]),
                       cfg["batch_size"], int(fx["seed"]), int(fx["lengths"].sum()))
    return (head + np.ascontiguousarray(game_priority, dtype=np.float32).tobytes()
            + np.ascontiguousarray(fx["lengths"], dtype=np.int32).tobytes()
            + np.ascontiguousarray(priorities, dtype=np.float32).tobytes())


@pytest.mark.parametrize("name", NAMES)
def test_shared_sampler_reproduces_g12_and_numpy_stream(check, name):
    ro = importlib.import_module("replay_oracle")
    fx = load_golden(f"g12_replay_{name}")
    cfg = cfg_of(fx)
    if cfg["PER"]:
        priorities, game_priority = fx["priorities"], fx["game_priority"]
    else:
        priorities = np.ones((len(fx["lengths"]), fx["root_values"].shape[1]), dtype=np.float32)
        game_priority = np.ones(len(fx["lengths"]), dtype=np.float32)
    out = check("batch", batch_payload(fx, cfg, priorities, game_priority))
    index = np.stack([out["game_index"], out["position"]], axis=1)
    assert np.array_equal(index, fx["index_batch"])
    if cfg["PER"]:
        assert np.array_equal(f32_of_bits(out["weight"]).view(np.uint32), fx["weight_batch"].view(np.uint32))
    # absorbing actions: where the fixture's batch passes the end of the game, the action is the draw
    U1 = cfg["num_unroll_steps"] + 1
    absorbing = np.array(out["absorbing"]).reshape(-1, U1)
    for b, (g, pos) in enumerate(fx["index_batch"]):
        for u in range(U1):
            if pos + u > fx["lengths"][g]:
                assert absorbing[b, u] == fx["action_batch"][b, u]
            else:
                assert absorbing[b, u] == 0
    # numpy's own generator through the same draws: same key block, same position
    games = games_of(fx, ro)
    for g, game in enumerate(games):
        game.priorities = priorities[g, : fx["lengths"][g]]
        game.game_priority = game_priority[g]
    rng = NumpyRng(int(fx["seed"]))
    ro.get_batch(games, cfg, rng)
    state = rng.rs.get_state()
    assert out["pos"] == state[2] and np.array_equal(np.array(out["key"], dtype=np.uint32), state[1])
    assert out["words"] > 2 * cfg["batch_size"] * (1 if cfg["PER"] else 0)


def test_priority_update_equals_sequential_loop(check):
    rs = np.random.RandomState(11)
    for trial in range(20):
        G, stride, steps, batch = int(rs.randint(2, 12)), 30, int(rs.randint(1, 13)), int(rs.randint(1, 80))
        oldest = int(rs.randint(0, 50))
        length = rs.randint(1, stride + 1, size=G).astype(np.int32)
        priorities = rs.uniform(0, 2, size=(G, stride)).astype(np.float32)
        # ids from a few below the oldest stored game (evicted) to the newest; few games, so they repeat and overlap
        ids = rs.randint(max(0, oldest - 3), oldest + G, size=batch).astype(np.int64)
        positions = np.array([rs.randint(0, length[g - oldest]) if g >= oldest else rs.randint(0, stride) for g in ids],
                             dtype=np.int32)
        fresh = rs.choice(np.array([0, 1e-12, 1e3, 0.5, 0.25], dtype=np.float32), size=(batch, steps)).astype(np.float32)
        fresh += (rs.random_sample((batch, steps)) < 0.5).astype(np.float32) * rs.random_sample((batch, steps)).astype(np.float32)
        payload = (struct.pack("<iiiiq", G, stride, steps, batch, oldest) + length.tobytes() + priorities.tobytes()
                   + ids.tobytes() + positions.tobytes() + fresh.tobytes())
        out = check("update", payload)
        want, want_game = priorities.copy(), np.full(G, -1, dtype=np.float32)
        for i in range(batch):                                   # replay_buffer.py:197-220
            g = int(ids[i]) - oldest
            if g < 0:
                continue
            row = want[g, : length[g]]
            end = min(positions[i] + steps, len(row))
            row[positions[i]: end] = fresh[i, : end - positions[i]]
            want_game[g] = np.max(row)
        assert np.array_equal(f32_of_bits(out["priorities"]).reshape(G, stride), want), trial
        assert np.array_equal(f32_of_bits(out["game_priority"]), want_game), trial


def test_sampler_entries_are_declared_exported_and_guarded(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    header = open(os.path.join(ROOT, "include", "mzreplay.h")).read()
    for name in ("mzreplay_sampler_enable", "mzreplay_sampler_get_rng", "mzreplay_sampler_set_rng", "mzreplay_set_priorities",
                 "mzreplay_get_priorities", "mzreplay_sample_batch", "mzreplay_make_batch_device",
                 "mzreplay_update_priorities"):
        assert name + "(" in header and name in native.PROTOTYPES and hasattr(lib, name)
    assert lib.mzmcts_abi_version() == 2
    # without a store nothing is touched
    assert lib.mzreplay_sampler_enable(None, 0, 0) != 0
    assert lib.mzreplay_sample_batch(None, 4, 0, 1, 1, 1, None, None, None, None, None, None) != 0
    assert lib.mzreplay_update_priorities(None, 4, None, None, None, None) != 0
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    import inspect
    assert "device_sampling" in inspect.signature(rb_mod.ReplayBuffer.__init__).parameters
    assert hasattr(importlib.import_module("muzero-hypermodel_amd.trainer").Trainer, "train_steps")
