"""csrc/replay_filer.h -- the index arithmetic of filing finished self-play games into the replay store on the device
(include/mzreplay.h mzreplay_filer_file) -- built for the host with g++ (tests/replay_filer_check.cpp) and held to the
host path it must equal:

* random move batches through the REAL host filer (self_play.HistoryFiler: pure host code) and a Python restatement of
  ReplayBuffer._add: which moves an env played, the order the finished games leave in, their ids and slots, which of them
  survive a call that wraps the ring, and all four store-wide counters;
* the C ABI of the feature: declared, exported, bound; mzreplay_file_moves laid out as a probe compiled against the
  header says; the filer refuses a null store with a message.

The device build of the same header is checked on the GPU by tests/test_gpu_replay_filer.py."""
import ctypes
import importlib
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
NEW_SYMBOLS = ("mzreplay_filer_create", "mzreplay_filer_destroy", "mzreplay_filer_begin", "mzreplay_filer_set_counters",
               "mzreplay_filer_file", "mzreplay_filer_sync", "mzreplay_filer_lengths", "mzreplay_filer_priorities",
               "mzreplay_read_games", "mzmcts_moves_device_ring", "mzmcts_moves_inputs_device_ring")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    work = tmp_path_factory.mktemp("replay_filer")
    exe = str(work / "replay_filer_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "replay_filer_check.cpp")],
                   check=True)

    def run(E, M, capacity, max_moves, chunk, counters, running, slot_length, actions, done):
        path = str(work / "call.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<5i4q", E, M, capacity, max_moves, chunk, *counters))
            for a, dtype in ((running, np.int32), (slot_length, np.int32), (actions, np.int32), (done, np.uint8)):
                f.write(np.ascontiguousarray(a, dtype=dtype).tobytes())
        proc = subprocess.run([exe, path], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        return json.loads(proc.stdout.strip().splitlines()[-1])
    return run


class HostStore:
    """ReplayBuffer._add's bookkeeping (replay_buffer.py), game by game, without the device."""

    def __init__(self, capacity, next_id=0):
        self.capacity, self.num_played_games, self.num_played_steps, self.total_samples = capacity, next_id, 0, 0
        self.buffer = {}
        self.slot_id = {}

    def add(self, lengths):
        ids = []
        for n in lengths:
            self.buffer[self.num_played_games] = int(n)
            self.slot_id[self.num_played_games % self.capacity] = self.num_played_games
            ids.append(self.num_played_games)
            self.num_played_games += 1
            self.num_played_steps += int(n)
            self.total_samples += int(n)
            if self.capacity < len(self.buffer):
                del_id = self.num_played_games - len(self.buffer)
                self.total_samples -= self.buffer[del_id]
                del self.buffer[del_id]
        return ids

    def counters(self):
        return [self.num_played_games, len(self.buffer), self.total_samples, self.num_played_steps]

    def slot_length(self):
        out = np.zeros(self.capacity, np.int32)
        for gid, n in self.buffer.items():
            out[gid % self.capacity] = n
        return out


def random_batch(rs, E, M, L, running, done_rate, stall_rate):
    """actions [M, E] (-1 from an env's first unplayed move on, garbage behind it) and done flags [M, E] that respect
    max_moves: a game is over at L moves at the latest."""
    actions = rs.randint(0, 3, size=(M, E)).astype(np.int32)
    done = np.zeros((M, E), np.uint8)
    for e in range(E):
        if rs.random_sample() < stall_rate:
            k = rs.randint(0, M + 1)
            if k < M:
                actions[k, e] = -1
                actions[k + 1:, e] = rs.randint(-1, 3, size=M - k - 1)   # undefined past the first unplayed move
        length = int(running[e])
        for m in range(M):
            length += 1
            if length >= L or rs.random_sample() < done_rate:
                done[m, e] = 1
                length = 0
    return actions, done


def run_case(check, seed):
    """Eight calls on one store and one host filer; returns which of the cases that matter the draws reached."""
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    rs = np.random.RandomState(100 + seed)
    E = int(rs.randint(1, 301))
    L, A, S = int(rs.randint(2, 9)), 2, 10
    capacity = int(rs.choice([1, 2, 3, 5, 17, 64, 1000]))
    store = HostStore(capacity, next_id=int(rs.choice([0, 7, 1234567])))
    filer = sp.HistoryFiler(E, L, (1, 1, 1), A)
    filer.begin(np.zeros((E, 1, 1, 1), np.float32))
    wrapped_once = wrapped_more = stalled = several = False
    for call in range(8):
        M = int(rs.randint(1, 17))
        running = filer.lengths().copy()
        actions, done = random_batch(rs, E, M, L, running, done_rate=float(rs.choice([0.0, 0.2, 0.7])),
                                     stall_rate=float(rs.choice([0.0, 0.3])))
        moves_done = np.array([next((m for m in range(M) if actions[m, e] < 0), M) for e in range(E)], np.int32)
        before, slot_length = store.counters(), store.slot_length()
        got = check(E, M, capacity, L, int(rs.choice([1, 7, 64, 1024])), before, running, slot_length, actions, done)
        # the host path: HistoryFiler files the batch, ReplayBuffer._add numbers and counts the games it hands out
        out = dict(moves_done=moves_done, actions=np.maximum(actions, 0), visits=np.ones((M, E, A), np.int32),
                   root_value_sum=np.zeros((M, E)))
        batch = filer.file(out, np.tile(np.arange(A, dtype=np.int32), (E, 1)), np.full(E, A, np.int32), S,
                           np.zeros((M, E), np.float32), done, np.zeros((M, E, 1, 1, 1), np.float32),
                           np.zeros((M, E, 1, 1, 1), np.float32))
        env = [] if batch is None else batch.env_index.tolist()
        lengths = [] if batch is None else batch.length.tolist()
        ids = store.add(lengths)
        assert got["refused"] == 0
        assert got["played"] == moves_done.tolist()
        assert got["env"] == env and got["length"] == lengths and got["id"] == ids
        assert got["slot"] == [i % capacity for i in ids]
        assert got["stored"] == [1 if i in store.buffer else 0 for i in ids]
        for j, gid in enumerate(ids):                    # a slot is written by the game that ends up owning it, once
            if got["stored"][j]:
                assert store.slot_id[gid % capacity] == gid
        assert got["counters"] == store.counters()
        assert got["running"] == filer.lengths().tolist()
        wrapped_once |= capacity < len(ids) <= 2 * capacity
        wrapped_more |= len(ids) > 2 * capacity
        stalled |= bool((moves_done < M).any())
        several |= len(env) != len(set(env))
    filer.close()
    return wrapped_once, wrapped_more, stalled, several


@pytest.mark.parametrize("seed", range(6))
def test_filing_order_ids_slots_and_counters_equal_the_host_path(check, pkg, seed):
    run_case(check, seed)


def test_the_random_batches_reach_the_cases_that_matter(check, pkg):
    seen = np.zeros(4, bool)
    for seed in range(6):
        seen |= np.array(run_case(check, seed))
    assert seen.all(), f"wrap once / wrap more than once / unplayed suffix / several games per env: {seen}"


def test_a_game_that_outgrows_max_moves_refuses_the_call(check):
    E, M, L = 3, 4, 3
    actions = np.zeros((M, E), np.int32)
    done = np.zeros((M, E), np.uint8)
    got = check(E, M, 8, L, 1024, [0, 0, 0, 0], np.zeros(E, np.int32), np.zeros(8, np.int32), actions, done)
    assert got["refused"] == 1 and got["env"] == [] and got["counters"] == [0, 0, 0, 0] and got["running"] == [0, 0, 0]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(pkg):
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("mzreplay.h", "mzmcts.h"))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in native.PROTOTYPES, f"{name} is not bound"


def test_file_moves_layout_matches_the_header(pkg, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    native = importlib.import_module("muzero-hypermodel_amd._native")
    fields = [name for name, _ in native.MzReplayFileMoves._fields_]
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include <cstddef>\n#include <cstdio>\n#include "mzreplay.h"\nint main() {\n'
                     '  std::printf("%zu", sizeof(mzreplay_file_moves));\n'
                     + "".join(f'  std::printf(" %zu", offsetof(mzreplay_file_moves, {name}));\n' for name in fields)
                     + "  return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, str(probe)], check=True)
    numbers = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert numbers[0] == ctypes.sizeof(native.MzReplayFileMoves)
    assert numbers[1:] == [getattr(native.MzReplayFileMoves, name).offset for name in fields]


def test_filer_create_fails_with_a_message_instead_of_crashing(pkg):
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    handle = ctypes.c_void_p()
    assert lib.mzreplay_filer_create(None, 4, ctypes.byref(handle)) != 0 and not handle.value
    assert b"mzreplay_filer_create" in lib.mzreplay_last_error(None)
    lib.mzreplay_filer_destroy(None)                     # a null filer is ignored
    assert lib.mzreplay_filer_file(None, None, None) != 0
    n = ctypes.c_int32()
    assert lib.mzreplay_filer_sync(None, ctypes.byref(n), None, None, None, None, None) != 0


def test_python_surface_exists(pkg):
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    rb = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    assert sp.FiledGames._fields == ("env_index", "length", "game_id")
    for name in ("file_to",):
        assert hasattr(sp.DeviceSelfPlay, name) and hasattr(sp.PipelinedDeviceSelfPlay, name)
    for name in ("attach_filer", "sync_filing", "download_games", "filer_lengths"):
        assert hasattr(rb.ReplayBuffer, name)
    with pytest.raises(NotImplementedError, match="file_to"):
        sp.PipelinedDeviceSelfPlay.file_to(object.__new__(sp.PipelinedDeviceSelfPlay), None)
