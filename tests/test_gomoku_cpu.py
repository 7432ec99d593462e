"""Gomoku, the parts that need no GPU: the host plugin and its config against fixture G18 (recorded from the
reference's games/gomoku.py), the shared rules header built for the host, the C oracle on 121-action traces, and the
argument check of mzenv_create."""
import ctypes
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from gomoku_cases import CELLS, TRACE_FILES, edge_boards, fixture_boards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


def gomoku():
    return importlib.import_module("muzero-hypermodel_amd.games.gomoku")


def test_host_plugin_replays_reference_playouts_g18(golden):
    """Every row of g18_gomoku_env bit for bit: observation (values and dtype of the array the plugin returns), legal
    list, to_play, reward and done (values and Python types), over 26 games: fives in all four directions, on the
    edges, a six, the second player's five, a full-board draw and runs that only wrap around a row end."""
    fx = golden("g18_gomoku_env")
    mod = gomoku()
    kinds = [str(k) for k in fx["kind"]]
    assert len(kinds) >= 24 and {"five_right", "five_down", "five_down_right", "five_down_left", "six", "wrap",
                                  "full_board_draw", "five_row0_corner", "five_second_player"} <= set(kinds)
    rows = 0
    for g in range(len(kinds)):
        idx = np.flatnonzero(fx["game"] == g)
        assert fx["step"][idx].tolist() == list(range(len(idx))) and len(idx) == fx["length"][g] + 1
        game = mod.Game(g)
        obs = game.reset()
        for r in idx:
            assert obs.dtype == np.float64 and np.array_equal(obs.astype(np.float32), fx["obs"][r]), (g, r)
            n = int(fx["n_legal"][r])
            assert game.legal_actions() == fx["legal"][r][:n].tolist() and (fx["legal"][r][n:] == -1).all()
            assert game.to_play() == fx["to_play"][r]
            rows += 1
            if fx["done"][r]:
                assert r == idx[-1]
                break
            action = int(fx["action"][r + 1])
            obs, reward, done = game.step(action)
            assert type(reward) is int and type(done) is bool
            assert reward == fx["reward"][r + 1] and done == bool(fx["done"][r + 1]), (g, r)
            assert game.action_to_string(action) == "ABCDEFGHIJK"[action // 11] + "ABCDEFGHIJK"[action % 11]
    assert rows == len(fx["game"])
    draw = kinds.index("full_board_draw")
    last = np.flatnonzero(fx["game"] == draw)[-1]
    assert fx["length"][draw] == 121 and fx["reward"][last] == 1 and fx["n_legal"][last] == 0
    with pytest.raises(NotImplementedError):
        mod.Game(0).expert_agent()


def test_config_equals_the_reference_field_by_field(golden):
    fx = golden("g18_gomoku_env")
    config = gomoku().MuZeroConfig()
    recorded = [k[len("config_"):] for k in fx.files if k.startswith("config_") and k != "config_temperatures"]
    assert set(recorded) == set(vars(config)) - {"results_path", "train_on_gpu"}
    for key in recorded:
        want = fx["config_" + key]
        got = getattr(config, key)
        if want.dtype.kind == "U":
            assert (got is None and str(want) == "None") or got == str(want), key
        elif want.ndim:
            assert list(got) == want.tolist(), key
        else:
            assert got == want.item() and type(got) is type(want.item()), key
    assert [config.visit_softmax_temperature_fn(t) for t in (0, 4999, 5000, 7499, 7500, 10000)] == fx["config_temperatures"].tolist()
    assert os.path.basename(os.path.dirname(config.results_path)) == "gomoku"


def test_shared_gomoku_rules_on_cpu(golden, tmp_path):
    """csrc/gomoku_rules.h + board_rules.h built for the host over every position of G18 and the hand-made edge boards
    (before and after their ply): finished, legal list, the random opponent's move, words consumed and stream state equal
    to HostStream's choice(n_legal); a full board has no move.  The per-stone test on the bordered board counts exactly
    the stones a numpy walk finds."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gomoku_rules_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "gomoku_rules_check.cpp"), "-lm"], check=True)
    fx = golden("g18_gomoku_env")
    boards, _ = fixture_boards(fx)
    rows = [(2000 + 7 * r, bool(fx["done"][r]), boards[r]) for r in range(len(boards))]
    mod = gomoku()
    for name, board, player, action, finished in edge_boards():
        env = mod.Gomoku()
        env.board = board.reshape(11, 11).astype("int32")
        env.player = player
        rows.append((3000 + len(rows), env.is_finished(), board))
        _, reward, done = env.step(action)
        assert done is finished and reward == int(finished), name          # the hand-stated verdicts hold on the host plugin
        rows.append((3000 + len(rows), finished, env.board.reshape(-1).astype(np.int8)))

    def five_starts(b):
        b = b.reshape(11, 11)
        count = 0
        for r in range(11):
            for c in range(11):
                for dr, dc in ((1, -1), (1, 0), (1, 1), (0, 1)):
                    cells = [(r + k * dr, c + k * dc) for k in range(5)]
                    if b[r, c] != 0 and all(0 <= x < 11 and 0 <= y < 11 and b[x, y] == b[r, c] for x, y in cells):
                        count += 1
                        break
        return count

    text = "\n".join(" ".join(map(str, [seed, int(fin), int((b == 0).sum())] + b.tolist() + np.flatnonzero(b == 0).tolist()))
                     for seed, fin, b in rows)
    proc = subprocess.run([exe], input=text, capture_output=True, text=True)
    report = json.loads(proc.stdout.strip().splitlines()[-1])
    assert proc.returncode == 0 and report["rows"] == len(rows), proc.stdout
    for key in ("finished_mismatches", "legal_mismatches", "random_mismatches", "stream_mismatches", "full_board_mismatches"):
        assert report[key] == 0, proc.stdout
    assert report["full_boards"] == 2                                       # G18's draw and the edge case's
    assert report["five_starts"] == sum(five_starts(b) for _, _, b in rows) > 20


def test_oracle_replays_gomoku_traces_bit_exact(oracle, golden):
    """The C oracle in injected mode on 121-action searches of real Gomoku positions (masked roots from 121 down to 3
    legal cells, both players, 30 simulations; one at the config's 400): noise, visits, value sums, per-simulation
    paths, tie-list sizes and stream word counts are the reference's."""
    from test_oracle_mcts import replay_trace
    small = golden(TRACE_FILES[0][1])
    assert small["n_legal"].min() <= 5 and small["n_legal"].max() == CELLS and set(small["to_play"].tolist()) == {0, 1}
    for simulations, name in TRACE_FILES:
        fx = golden(name)
        assert int(fx["cfg_A"]) == CELLS and int(fx["cfg_S"]) == simulations
        for i in range(len(fx["seed"])):
            tree, rng, noise, n = replay_trace(oracle, fx, i)
            st = tree.root_stats()
            assert np.array_equal(noise[:n], fx["noise"][i][:n]), i
            assert np.array_equal(st["visits"], fx["visits"][i][:n]), i
            assert np.array_equal(st["child_value_sum"], fx["child_value_sum"][i][:n]), i
            assert np.array_equal(st["child_prior"], fx["child_prior"][i][:n]), i
            assert st["root_value_sum"] == fx["root_value_sum"][i] and st["root_visit"] == int(fx["cfg_S"])
            assert st["max_tree_depth"] == fx["max_tree_depth"][i]
            assert st["mms_min"] == fx["mms_min"][i] and st["mms_max"] == fx["mms_max"][i]
            assert np.array_equal(tree.sim_depth, fx["sim_depth"][i])
            assert np.array_equal(tree.sim_actions, fx["sim_actions"][i])
            assert np.array_equal(tree.sim_ties, fx["sim_ties"][i])
            assert rng.words == fx["rng_words_run"][i]
            cv, rv = tree.search_statistics()
            assert np.array_equal(cv, fx["child_visits_target"][i]) and rv == fx["root_value_target"][i]
            slot = oracle.select_action(rng, st["visits"], float(fx["temperature"][i]))
            assert int(fx["legal"][i][slot]) == fx["action_T"][i]
            assert rng.words == fx["rng_words_run"][i] + fx["rng_words_select"][i]


def test_mzenv_create_knows_gomoku(pkg):
    """Game id 3 gets past mzenv_create's argument check (without a device the error is the missing device, not the
    argument; id 4 is still refused), and the Python layers name it."""
    native = importlib.import_module("muzero-hypermodel_amd._native")
    device = importlib.import_module("muzero-hypermodel_amd.games.device")
    assert device.GAME_IDS["gomoku"] == 3 and device.MAX_EPISODE_STEPS["gomoku"] == 121
    lib = native.load()
    seeds = np.zeros(2, dtype=np.uint32)
    handle = ctypes.c_void_p()
    assert lib.mzenv_create(4, 2, 0, native.ptr(seeds, native.c_u32_p), ctypes.byref(handle)) == -1
    assert b"bad argument" in lib.mzenv_last_error(None)
    rc = lib.mzenv_create(3, 2, 0, native.ptr(seeds, native.c_u32_p), ctypes.byref(handle))
    if rc == 0:                                  # a machine with a device: the env exists and has Gomoku's shape
        a, p, shape = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 3)()
        lib.mzenv_shape(handle, ctypes.byref(a), ctypes.byref(p), shape)
        lib.mzenv_destroy(handle)
        assert (a.value, p.value, tuple(shape)) == (121, 2, (3, 11, 11))
    else:
        assert rc == -2 and b"no HIP device" in lib.mzenv_last_error(None)
