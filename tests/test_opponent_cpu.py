"""Evaluation games against a scripted opponent, the parts that need no GPU: the shared board rules (the text the
environment kernels compile) against fixture G11, the history filer's opponent plies against a numpy restatement, and
the argument checks of the environments' opponent mode."""
import ctypes
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


def g11_positions(golden, name):
    """Every non-terminal position of fixture G11: (game id 1|2, player +1|-1, numpy seed, expert's move, board)."""
    fx = golden(f"g11_{name}_env")
    rows = []
    for r in range(len(fx["game"])):
        if fx["done"][r]:
            continue
        obs = fx["obs"][r]
        board = (obs[0] - obs[1]).astype(np.int8).reshape(-1)          # planes: first player's stones, second's, side to move
        rows.append((1 if name == "tictactoe" else 2, int(obs[2].flat[0]), 1000 + 31 * int(fx["game"][r]) + int(fx["step"][r]),
                     int(fx["expert"][r]), board))
    return rows


def test_shared_board_rules_replay_g11_experts_on_cpu(golden, tmp_path):
    """csrc/board_rules.h built for the host: in all 818 non-terminal positions of G11's playouts the expert's move is
    the reference's (column `expert`, recorded with numpy seeded 1000 + 31 * game + step), the random opponent's is
    legal[choice(n)], and words consumed / stream position / key block equal HostStream's for choice(n_legal).  A full
    board yields no move and draws nothing (the environment kernels then leave the env alone)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "board_rules_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "board_rules_check.cpp"), "-lm"], check=True)
    rows = g11_positions(golden, "tictactoe") + g11_positions(golden, "connect4")
    text = "\n".join(" ".join(map(str, [g, p, seed, want] + board.tolist())) for g, p, seed, want, board in rows)
    proc = subprocess.run([exe], input=text, capture_output=True, text=True)
    report = json.loads(proc.stdout.strip().splitlines()[-1])
    assert proc.returncode == 0 and report["rows"] == 818, proc.stdout
    assert report["expert_mismatches"] == report["stream_mismatches"] == report["random_mismatches"] == 0, proc.stdout
    assert report["full_board_mismatches"] == 0, proc.stdout


def test_history_filer_files_opponent_plies(pkg):
    """A batch mixing searched and opponent plies (empty legal set + `played`), games ending on either kind: the packed
    games equal a numpy restatement; history(i) has None exactly on the opponent plies and as many child_visits rows as
    searched plies.  Without `played` an empty legal set is filed as before."""
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    E, M, A, S, L = 5, 12, 4, 10, 6
    rs = np.random.RandomState(3)
    obs_shape = (1, 2, 2)
    out = dict(actions=rs.randint(0, A, (M, E)).astype(np.int32), visits=rs.randint(0, S, (M, E, A)).astype(np.int32),
               root_value_sum=rs.randn(M, E), moves_done=np.full(E, M, np.int32))
    num_legal = rs.randint(1, A + 1, (M, E)).astype(np.int32)
    opponent = rs.rand(M, E) < 0.45
    num_legal[opponent] = 0
    out["actions"][opponent] = -1
    legal = np.stack([np.stack([rs.permutation(A) for _ in range(E)]) for _ in range(M)]).astype(np.int32)
    played = np.where(opponent, rs.randint(0, A, (M, E)), out["actions"]).astype(np.int32)
    done = (rs.rand(M, E) < 0.3).astype(np.uint8)
    done[5] = 1                                                  # (no game outgrows L = 6)
    done[11] = 1
    assert (done & opponent).any() and (done & ~opponent).any()  # games end on either kind of ply
    rewards = rs.randn(M, E).astype(np.float32)
    obs_after = rs.randn(M, E, *obs_shape).astype(np.float32)
    obs_next = rs.randn(M, E, *obs_shape).astype(np.float32)
    tp = rs.randint(0, 2, (M, E)).astype(np.int32)
    first = rs.randn(E, *obs_shape).astype(np.float32)
    filer = sp.HistoryFiler(E, L, obs_shape, A)
    filer.begin(first, np.zeros(E, np.int32))
    batch = filer.file(out, legal, num_legal, S, rewards, done, obs_after, obs_next, to_play_after=1 - tp, to_play_next=tp,
                       played=played)
    games = {}
    for i in range(len(batch)):
        games.setdefault(int(batch.env_index[i]), []).append(i)
    for e in range(E):
        start_obs, start_tp, rows, want = first[e], 0, [], []
        for m in range(M):
            rows.append(m)
            if done[m, e]:
                want.append((start_obs, start_tp, rows))
                start_obs, start_tp, rows = obs_next[m, e], tp[m, e], []
        assert len(games[e]) == len(want)
        for i, (obs0, tp0, ms) in zip(games[e], want):
            n = len(ms)
            assert batch.length[i] == n
            gh = batch.history(i)
            assert np.array_equal(gh.observation_history[0], obs0) and gh.to_play_history[0] == tp0
            assert gh.action_history == [0] + [int(played[m, e]) for m in ms]
            assert gh.reward_history == [0.0] + [float(rewards[m, e]) for m in ms]
            assert gh.to_play_history[1:] == [int(1 - tp[m, e]) for m in ms]
            assert [v is None for v in gh.root_values] == [bool(opponent[m, e]) for m in ms]
            searched = [m for m in ms if not opponent[m, e]]
            assert len(gh.child_visits) == len(searched)
            for row, m in zip(gh.child_visits, searched):
                cv = np.zeros(A)
                cv[legal[m, e, : num_legal[m, e]]] = out["visits"][m, e, : num_legal[m, e]] / S
                assert row == cv.tolist()
            assert [v for v in gh.root_values if v is not None] == [out["root_value_sum"][m, e] / S for m in searched]
            # the packed arrays keep a slot per ply: NaN / a zero row on the opponent's
            rv = batch.root_values[i, :n]
            assert np.array_equal(np.isnan(rv), opponent[ms, e]) and not batch.child_visits[i, :n][opponent[ms, e]].any()
    assert filer.searched_moves() == int((~opponent).sum())     # every env filed all M plies
    # a NaN that came out of a search (its child_visits row is not zero) is not taken for an opponent's ply
    searched_at = [(i, j) for i in range(len(batch)) for j in range(int(batch.length[i]))
                   if not np.isnan(batch.root_values[i, j]) and batch.child_visits[i, j].any()]
    i, j = searched_at[0]
    batch.root_values[i, j] = np.nan
    with pytest.raises(ValueError, match="searched ply has a NaN root value"):
        batch.history(i)
    # without `played` nothing changes for an empty legal set: the search's own action, a zero root value sum / S
    filer2 = sp.HistoryFiler(E, L, obs_shape, A)
    filer2.begin(first, np.zeros(E, np.int32))
    plain = filer2.file(out, legal, num_legal, S, rewards, done, obs_after, obs_next, to_play_after=1 - tp, to_play_next=tp)
    assert not np.isnan(plain.root_values[:, : int(plain.length.min())]).any()
    assert plain.history(0).action_history[1:] == [int(out["actions"][m, int(plain.env_index[0])])
                                                    for m in range(int(plain.length[0]))]


def test_opponent_mode_argument_checks_need_no_device(pkg):
    """mzenv_set_opponent judges its arguments before anything else: an unknown kind and missing stream pointers are
    refused with their own messages, with or without a device (no env exists here: nothing can be launched)."""
    lib = importlib.import_module("muzero-hypermodel_amd._native").load()
    key, pos = (ctypes.c_uint32 * 624)(), (ctypes.c_int32 * 1)()
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.mzenv_set_opponent(None, 7, 0, addr(key), addr(pos)) == -1
    assert b"unknown opponent kind" in lib.mzenv_last_error(None)
    for k, p in ((None, addr(pos)), (addr(key), None), (None, None)):
        assert lib.mzenv_set_opponent(None, 1, 0, k, p) == -1
        assert b"streams it draws from" in lib.mzenv_last_error(None)
    assert lib.mzenv_set_opponent(None, 2, 0, addr(key), addr(pos)) == -1
    assert b"null handle" in lib.mzenv_last_error(None)
    assert lib.mzenv_step_opponent(None, None, None, None, None, None, None) == -1
    assert lib.mzenv_advance_opponent(*([None] * 12)) == -1
    assert lib.mzenv_set_boards(None, None, None) == -1
    assert lib.mzmcts_rng_streams(None, None, None) != 0 and lib.mzmcts_rng_consumed(None, None) != 0
    assert lib.mzmcts_moves_sit_out(None, 1) != 0
