"""TwentyOne and SimpleGrid, the parts that need no GPU: the host plugins and their configs against fixture G23
(recorded from the reference's games/twentyone.py and games/simple_grid.py), the shared rules header built for the host,
and the argument check of mzenv_create.  Every comparison is on integers or integer-valued floats and is exact."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from solo_cases import as_obs, grid_obs, play_host, plugin, t21_obs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
TEMPERATURE_STEPS = (0, 499999, 500000, 749999, 750000, 1000000)


def check_t21_observation(observation, hands):
    """The reference's types: a list of two float32 planes and an integer plane; numpy.array of it has shape (3,3,3)."""
    assert isinstance(observation, list) and [str(o.dtype) for o in observation] == ["float32", "float32", "int64"]
    assert np.array(observation).shape == (3, 3, 3)
    assert np.array_equal(as_obs("twentyone", observation), t21_obs(hands))


def test_twentyone_plugin_replays_g23(golden):
    """64 games Game(e) x 400 plies, finished games reset in place: hands, reward, done (values and Python types),
    observation and the plugin's stream position after the constructor, every reset and every ply."""
    fx = dict(golden("g23_twentyone_env"))            # (every array unpacked once: the loop reads them per ply)
    mod = plugin("twentyone")
    E, T = fx["action"].shape
    assert (E, T) == (64, 400)
    for e in range(E):
        game = mod.Game(int(fx["seed"][e]))
        env = game.env
        position = lambda: int(env.random.get_state()[2])
        assert [env.player_hand, env.dealer_hand] == fx["ctor_hands"][e].tolist() and position() == fx["ctor_pos"][e]
        check_t21_observation(game.reset(), fx["first_hands"][e])
        assert position() == fx["first_pos"][e]
        for t in range(T):
            observation, reward, done = game.step(int(fx["action"][e, t]))
            assert type(reward) is int and type(done) is bool, (e, t)
            assert reward == fx["reward"][e, t] and done == bool(fx["done"][e, t]), (e, t)
            assert [env.player_hand, env.dealer_hand] == fx["hands"][e, t].tolist(), (e, t)
            check_t21_observation(observation, fx["hands"][e, t])
            assert position() == fx["pos"][e, t], (e, t)
            assert game.legal_actions() == [0, 1] and game.to_play() == 0
            if done:
                check_t21_observation(game.reset(), fx["next_hands"][e, t])
            assert [env.player_hand, env.dealer_hand] == fx["next_hands"][e, t].tolist(), (e, t)
            assert position() == fx["next_pos"][e, t], (e, t)
    assert mod.Game(0).action_to_string(0) == "0. Hit" and mod.Game(0).action_to_string(1) == "1. Stand"


def test_simple_grid_plugin_replays_g23(golden):
    """All 2^6 six-ply action sequences and the 12 illegal moves along the bottom row: position, reward, done (values
    and Python types) and observation; legal_actions() is [0, 1] in every state."""
    fx = dict(golden("g23_simple_grid_env"))
    mod = plugin("simple_grid")
    assert len(fx["length"]) == 65 and fx["length"][64] == 15
    rows = 0
    for s in range(len(fx["length"])):
        idx = np.flatnonzero(fx["seq"] == s)
        assert fx["step"][idx].tolist() == list(range(1, len(idx) + 1)) and len(idx) == fx["length"][s]
        game = mod.Game(s)
        observation = game.reset()
        assert np.array_equal(as_obs("simple_grid", observation), grid_obs(0, 0))
        for r in idx:
            observation, reward, done = game.step(int(fx["action"][r]))
            assert type(reward) is int and type(done) is bool
            assert reward == fx["reward"][r] and done == bool(fx["done"][r]), (s, r)
            assert game.env.position == [fx["row"][r], fx["col"][r]], (s, r)
            assert isinstance(observation, list) and observation[0][0].dtype == np.float64
            assert np.array(observation).shape == (1, 1, 9)
            assert np.array_equal(as_obs("simple_grid", observation), grid_obs(fx["row"][r], fx["col"][r]))
            assert game.legal_actions() == [0, 1] and game.to_play() == 0
            assert done == ((fx["row"][r], fx["col"][r]) == (2, 2))
            rows += 1
    assert rows == len(fx["seq"])
    assert mod.Game(0).action_to_string(0) == "0. Down" and mod.Game(0).action_to_string(1) == "1. Right"


@pytest.mark.parametrize("name", ["twentyone", "simple_grid"])
def test_config_equals_the_reference_field_by_field(golden, name):
    fx = golden(f"g23_{name}_env")
    config = plugin(name).MuZeroConfig()
    recorded = [k[len("cfg_"):] for k in fx.files if k.startswith("cfg_") and k != "cfg_temperatures"]
    assert set(recorded) == set(vars(config)) - {"results_path", "train_on_gpu"}
    for key in recorded:
        want = fx["cfg_" + key]
        got = getattr(config, key)
        if want.dtype.kind == "U":
            assert (got is None and str(want) == "None") or got == str(want), key
        elif want.ndim:
            assert list(got) == want.tolist(), key
        else:
            assert got == want.item() and type(got) is type(want.item()), key
    got = [config.visit_softmax_temperature_fn(t) for t in TEMPERATURE_STEPS]
    assert got == fx["cfg_temperatures"].tolist()
    assert got == ([1.0, 1.0, 0.5, 0.5, 0.25, 0.25] if name == "twentyone" else [1] * 6)
    assert [config.visit_softmax_temperature_fn(t) for t in (0, 500e3, 750e3)] == \
        ([1.0, 0.5, 0.25] if name == "twentyone" else [1, 1, 1])
    assert os.path.basename(os.path.dirname(config.results_path)) == name


@pytest.fixture(scope="module")
def rules_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("solo") / "solo_rules_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "solo_rules_check.cpp"), "-lm"], check=True)

    def run(lines):
        proc = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        out = [np.array(line.split(), dtype=np.int64) for line in proc.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def test_shared_rules_replay_g23_twentyone(golden, rules_check):
    """csrc/solo_rules.h built for the host replays every G23 env from its seed: hands, rewards, done flags, stream
    positions and word counts -- the constructor's, every reset's and every ply's -- equal the fixture."""
    fx = dict(golden("g23_twentyone_env"))
    E, T = fx["action"].shape
    lines = [" ".join(map(str, ["T", int(fx["seed"][e]), 0, T] + fx["action"][e].tolist())) for e in range(E)]
    for e, row in enumerate(rules_check(lines)):
        head, plies = row[:8], row[8:].reshape(T, 11)
        assert head.tolist() == [*fx["ctor_hands"][e], fx["ctor_words"][e], fx["ctor_pos"][e],
                                 *fx["first_hands"][e], fx["first_words"][e], fx["first_pos"][e]], e
        want = np.column_stack([fx["hands"][e], fx["reward"][e], fx["done"][e], fx["words"][e], fx["pos"][e], fx["ply"][e],
                                fx["next_hands"][e], fx["reset_words"][e], fx["next_pos"][e]])
        assert np.array_equal(plies, want), (e, np.flatnonzero((plies != want).any(axis=1))[:5])
    assert (fx["words"].sum(axis=1) + fx["reset_words"].sum(axis=1) > 1000).all()     # every stream was regenerated


def test_shared_rules_replay_g23_simple_grid(golden, rules_check):
    fx = dict(golden("g23_simple_grid_env"))
    lines, idxs = [], []
    for s in range(len(fx["length"])):
        idx = np.flatnonzero(fx["seq"] == s)
        idxs.append(idx)
        lines.append(" ".join(map(str, ["G", 0, len(idx)] + fx["action"][idx].tolist())))
    for idx, row in zip(idxs, rules_check(lines)):
        plies = row.reshape(len(idx), 7)
        want = np.column_stack([fx["row"][idx], fx["col"][idx], fx["reward"][idx], fx["done"][idx], fx["step"][idx]])
        assert np.array_equal(plies[:, :5], want)
        after = np.where(fx["done"][idx][:, None] != 0, 0, want[:, :2])                # a finished game starts again at (0, 0)
        assert np.array_equal(plies[:, 5:], after)


def test_shared_rules_move_limit_and_skipped_turns(rules_check):
    """The limit rule: with max_moves = 1 a hit that neither busts nor reaches 21 ends the game with reward
    0, the dealer's hand as it was and no word beyond the hit's own card; the next game's cards follow.  SimpleGrid
    dawdling on illegal moves ends at ply 6 with reward 0.  A negative action leaves hands, stream and ply count alone.
    Everything equals the host plugins played under the same rules."""
    rs = np.random.RandomState(23)
    E, T = 16, 120
    actions = rs.randint(0, 2, size=(E, T))
    seeds = 100 + np.arange(E)
    rows = rules_check([" ".join(map(str, ["T", int(seeds[e]), 1, T] + actions[e].tolist())) for e in range(E)])
    host = play_host("twentyone", seeds, actions, max_moves=1)
    limited = 0
    for e, row in enumerate(rows):
        plies = row[8:].reshape(T, 11)
        assert np.array_equal(t21_obs(plies[:, :2]), host["obs_after"][:, e])
        assert np.array_equal(t21_obs(plies[:, 7:9]), host["obs_next"][:, e])
        assert np.array_equal(plies[:, 2], host["reward"][:, e]) and (plies[:, 3] == 1).all() and (plies[:, 6] == 1).all()
        before = np.vstack([row[4:6][None], plies[:-1, 7:9]])                         # hands each ply started from
        hit_on = (actions[e] == 0) & (plies[:, 0] < 21)
        limited += int(hit_on.sum())
        assert (plies[hit_on, 1] == before[hit_on, 1]).all() and (plies[hit_on, 2] == 0).all()
        # words of the stream: position differences equal the reported counts (mod one block)
        pos = np.concatenate([[row[7]], plies[:, [5, 10]].reshape(-1)])
        words = plies[:, [4, 9]].reshape(-1)
        assert np.array_equal((np.diff(pos) - words) % 624, np.zeros_like(words))
    assert limited > 400
    # negative actions: every third env sits five plies out
    skipping = actions.copy()
    skipping[::3, 10:15] = -1
    rows = rules_check([" ".join(map(str, ["T", int(seeds[e]), 0, T] + skipping[e].tolist())) for e in range(E)])
    host = play_host("twentyone", seeds, skipping)
    for e, row in enumerate(rows):
        plies = row[8:].reshape(T, 11)
        assert np.array_equal(t21_obs(plies[:, :2]), host["obs_after"][:, e])
        assert np.array_equal(plies[:, 2], host["reward"][:, e]) and np.array_equal(plies[:, 3], host["done"][:, e])
        skipped = skipping[e] < 0
        assert (plies[skipped, 4] == 0).all() and (plies[skipped, 9] == 0).all()
        assert np.array_equal(np.where(plies[:, 3] != 0, 0, plies[:, 6]), host["moves"][:, e])
    # SimpleGrid at its own limit: six plies of "down" end at (2, 0) with reward 0; a mixed walk ends at the goal
    grid = rules_check(["G 6 12 " + " ".join(["0"] * 12), "G 6 8 0 1 0 1 0 0 1 1"])
    assert grid[0].reshape(12, 7)[:, :5].tolist() == [[1, 0, 0, 0, 1], [2, 0, 0, 0, 2], [2, 0, 0, 0, 3], [2, 0, 0, 0, 4],
                                                      [2, 0, 0, 0, 5], [2, 0, 0, 1, 6]] * 2
    assert grid[1].reshape(8, 7)[:, :5].tolist() == [[1, 0, 0, 0, 1], [1, 1, 0, 0, 2], [2, 1, 0, 0, 3], [2, 2, 10, 1, 4],
                                                     [1, 0, 0, 0, 1], [2, 0, 0, 0, 2], [2, 1, 0, 0, 3], [2, 2, 10, 1, 4]]


def test_mzenv_create_knows_the_solo_games(pkg):
    """Game ids 5 and 6 get past mzenv_create's argument check (without a device the error is the missing device); ids 4
    and 7 are refused with "bad argument"; the Python layers name both games."""
    native = importlib.import_module("muzero-hypermodel_amd._native")
    device = importlib.import_module("muzero-hypermodel_amd.games.device")
    assert device.GAME_IDS["twentyone"] == 5 and device.GAME_IDS["simple_grid"] == 6
    assert device.MAX_EPISODE_STEPS["twentyone"] == 20
    assert device.MAX_EPISODE_STEPS["simple_grid"] > 10 ** 9                          # above any config.max_moves
    lib = native.load()
    seeds = np.zeros(2, dtype=np.uint32)
    handle = ctypes.c_void_p()
    for refused in (4, 7, -1):
        assert lib.mzenv_create(refused, 2, 0, native.ptr(seeds, native.c_u32_p), ctypes.byref(handle)) == -1
        assert b"bad argument" in lib.mzenv_last_error(None)
    for game, shape in ((5, (3, 3, 3)), (6, (1, 1, 9))):
        rc = lib.mzenv_create(game, 2, 0, native.ptr(seeds, native.c_u32_p), ctypes.byref(handle))
        if rc == 0:                                  # a machine with a device: the env exists and has the game's shape
            a, p, got = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 3)()
            lib.mzenv_shape(handle, ctypes.byref(a), ctypes.byref(p), got)
            lib.mzenv_destroy(handle)
            assert (a.value, p.value, tuple(got)) == (2, 1, shape)
        else:
            assert rc == -2 and b"no HIP device" in lib.mzenv_last_error(None)
