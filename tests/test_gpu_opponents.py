"""Evaluation games on device-resident envs: the scripted opponents of the environment kernels against fixture G11 and
numpy, reference games with opponents (fixture G6) through DeviceSelfPlay move by move and as move batches, many envs
against BatchedSelfPlay's host plugins, the temperature threshold over opponent plies, test mode of the training loop
and the public `evaluate`."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import load_golden, synthetic_model
from test_gpu_parity import G6_NEAR_TIES, RESNET_TOL
from test_opponent_cpu import g11_positions

pytestmark = pytest.mark.gpu


def games(name):
    return importlib.import_module(f"muzero-hypermodel_amd.games.{name}")


@pytest.fixture(scope="module")
def sp(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.self_play")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def game_config(name, fc=False):
    config = games(name).MuZeroConfig()
    if fc:
        config.network, config.encoding_size = "fullyconnected", 16
        config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
        config.num_simulations = min(config.num_simulations, 25)       # (the fused kernel keeps the trees in LDS)
    return config


# ---- the environment kernels alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tictactoe", "connect4"])
@pytest.mark.parametrize("kind", ["expert", "random"])
def test_opponent_step_in_every_g11_position(pkg, name, kind):
    """Every non-terminal position of G11's playouts set up on a device env, its stream seeded as the fixture's numpy
    was: one opponent-mode step plays the reference expert's move (column `expert`) / numpy.random.choice's, reports the
    words numpy consumed, and the engine's mirror, told of them, stands where numpy's generator stands."""
    dev = importlib.import_module("muzero-hypermodel_amd.games.device")
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    rows = g11_positions(load_golden, name)
    E = len(rows)
    seeds = [r[2] for r in rows]
    config = game_config(name)
    engine = engine_mod.BatchedMCTS(config, E, device="cuda", seeds=seeds)
    envs = dev.DeviceEnvs(name, E, seeds=seeds)
    boards, players = np.stack([r[4] for r in rows]), [r[1] for r in rows]
    envs.set_boards(boards, players)
    # every env's side to move is the opponent's: MuZero plays the other one
    tp = np.array([0 if r[1] == 1 else 1 for r in rows])
    want, want_words, want_state = [], [], []
    for g, player, seed, expert, board in rows:
        legal = np.flatnonzero(board == 0) if name == "tictactoe" else np.flatnonzero(board.reshape(6, 7)[5] == 0)
        np.random.seed(seed)
        pick = int(np.random.choice(legal))
        want.append(expert if kind == "expert" else pick)
        want_state.append(np.random.get_state())
        # a fresh seed leaves the position at 624; the first word regenerates the block and counts from 0
        want_words.append(want_state[-1][2] % 624)
    for mzp in (0, 1):
        envs.set_opponent(kind, mzp, engine)
        obs, legal, num_legal, to_play = envs.observe()
        mine = tp == mzp
        assert ((num_legal.cpu().numpy() == 0) == ~mine).all()
        assert np.array_equal(to_play.cpu().numpy(), tp)
    # step the envs whose opponent is to move under muzero_player = 1 - to_play: two calls, each leaves the others alone
    # (and their streams: every env draws once, from the state its seed gives)
    played = np.full(E, -1)
    words = np.zeros(E, np.uint32)
    for mzp in (0, 1):
        envs.set_boards(boards, players)                       # (the first call's envs go back to their position)
        envs.set_opponent(kind, mzp, engine)
        envs.step(np.full(E, -1, np.int32))
        torch.cuda.synchronize()
        sel = tp != mzp
        got = envs.played.cpu().numpy()
        assert (got[~sel] == -1).all()                         # MuZero's turn with action -1: untouched
        played[sel] = got[sel]
        words[sel] = envs.words.cpu().numpy().view(np.uint32)[sel]
        assert (envs.words.cpu().numpy()[~sel] == 0).all()
    assert played.tolist() == want
    assert words.tolist() == want_words                        # the words numpy's choice consumed, env by env
    engine.rng_consumed(words)
    for e in range(E):
        state, ref = engine.get_rng_state(e), want_state[e]
        assert state[2] == ref[2] and np.array_equal(state[1], ref[1]), e
    n_legal = np.array([len(np.flatnonzero(r[4] == 0)) if name == "tictactoe" else int((r[4].reshape(6, 7)[5] == 0).sum())
                        for r in rows])
    assert (words[n_legal == 1] == 0).all() and (words[n_legal > 1] >= 1).all()    # a single legal action consumes no word
    # a finished, un-reset game: on a full board the opponent has no move -- the env is left alone, nothing is drawn
    full = np.where((np.arange(boards.shape[1]) // 2) % 2 == 1, 1, -1).astype(np.int8)
    envs.set_boards(np.tile(full, (E, 1)), players)
    for mzp in (0, 1):
        envs.set_opponent(kind, mzp, engine)
        reward, done = envs.step(np.full(E, 3, np.int32))
        torch.cuda.synchronize()
        sel = tp != mzp
        assert (envs.played.cpu().numpy()[sel] == -1).all() and (envs.words.cpu().numpy() == 0).all()
        assert not reward.cpu().numpy()[sel].any() and not done.cpu().numpy()[sel].any()
        board_now = (envs.observe()[0].cpu().numpy()[:, 0] - envs.observe()[0].cpu().numpy()[:, 1]).reshape(E, -1)
        assert np.array_equal(board_now[sel], np.tile(full, (int(sel.sum()), 1)))
        envs.set_boards(np.tile(full, (E, 1)), players)
    envs.close()
    engine.close()


def test_opponent_mode_refuses_cartpole_and_plain_calls(pkg):
    dev = importlib.import_module("muzero-hypermodel_amd.games.device")
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    cart = dev.DeviceEnvs("cartpole", 4)
    engine = engine_mod.BatchedMCTS(game_config("cartpole"), 4, device="cuda", seeds=[0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="one-player game has no opponent"):
        cart.set_opponent("expert", 0, engine)
    with pytest.raises(NotImplementedError):
        cart.set_opponent("human", 0, engine)
    cart.close()
    engine.close()
    ttt = dev.DeviceEnvs("tictactoe", 4)
    engine = engine_mod.BatchedMCTS(game_config("tictactoe"), 4, device="cuda", seeds=[0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="muzero_player is not a player"):
        ttt.set_opponent("random", 2, engine)
    ttt.set_opponent("random", 1, engine)
    lib = ttt._lib
    a = ttt._actions
    assert lib.mzenv_step(ttt._h, a.data_ptr(), ttt.reward.data_ptr(), ttt.done.data_ptr(), None) == -1
    assert b"mzenv_step_opponent" in lib.mzenv_last_error(ttt._h)
    ttt.set_opponent("self")
    ttt.step(np.zeros(4, np.int32))
    assert ttt.to_play.cpu().numpy().tolist() == [0] * 4 and ttt.observe()[3].cpu().numpy().tolist() == [1] * 4
    ttt.close()
    engine.close()


# ---- reference games with opponents (fixture G6) ----------------------------------------------------------------------
def check_against_g6(fx, run, gh, A, config, near_ties):
    assert gh.action_history == fx[f"run{run}_actions"].tolist(), run
    assert gh.reward_history == fx[f"run{run}_rewards"].tolist() and gh.to_play_history == fx[f"run{run}_to_play"].tolist()
    got_cv = np.array(gh.child_visits, dtype=np.float64).reshape(-1, A)
    ref_cv = fx[f"run{run}_child_visits"]
    got_rv = np.array([np.nan if v is None else v for v in gh.root_values])
    ref_rv = fx[f"run{run}_root_values"].copy()
    assert np.array_equal(np.isnan(got_rv), np.isnan(ref_rv))                       # None exactly on the opponent's plies
    assert got_cv.shape == ref_cv.shape
    flipped = [m for m in range(len(got_cv)) if not np.array_equal(got_cv[m], ref_cv[m])]
    assert flipped == [m for m in near_ties.get(run, []) if m in flipped], (run, flipped)
    searched = np.flatnonzero(~np.isnan(ref_rv))
    for m in flipped:
        at = searched[m]
        assert abs(got_rv[at] - ref_rv[at]) <= 4.0 / config.num_simulations
        got_rv[at] = ref_rv[at]
    np.testing.assert_allclose(got_rv, ref_rv, rtol=0, atol=RESNET_TOL["value_tol"], equal_nan=True)
    assert np.array_equal(np.array(gh.observation_history, dtype=np.float32), fx[f"run{run}_observations"])


@pytest.mark.parametrize("fixture,game,runs", [("g6_tictactoe_games", "tictactoe", (4, 5)),
                                               ("g6_connect4_opponents_games", "connect4", (0, 1, 2))])
@pytest.mark.parametrize("form", ["step", "batches"])
def test_device_actor_replays_reference_opponent_games_g6(sp, models_mod, fixture, game, runs, form):
    """The reference's recorded test-mode games (expert / random opponent, MuZero as either player) through DeviceSelfPlay
    with one env, move by move and as play_moves batches: actions, rewards, players, policy targets and the None pattern
    exact, root values within the residual networks' bar -- and the env's stream afterwards where the reference's
    global generator was left (rng_pos_end / rng_next_word): the mirror accounting of the opponent's device draws."""
    config = game_config(game)
    A = len(config.action_space)
    _, weights = synthetic_model(models_mod, config, "cpu")
    fx = load_golden(fixture)
    near_ties = G6_NEAR_TIES.get((fixture, "split"), {})
    for run in runs:
        seed, temp, thr, opp, mzp = fx[f"run{run}_args"]
        opponent = {1: "expert", 2: "random"}[int(opp)]
        thr = None if thr < 0 else int(thr)
        actor = sp.DeviceSelfPlay({"weights": weights}, game, config, int(seed), 1)
        finished = []
        n = len(fx[f"run{run}_actions"]) - 1
        if form == "step":
            for _ in range(n):
                actor.step(float(temp), thr, on_game=lambda e, gh: finished.append(gh), opponent=opponent, muzero_player=int(mzp))
        else:
            left = n
            while left:
                m = min(left, 4)
                actor.play_moves(m, float(temp), on_game=lambda e, gh: finished.append(gh), temperature_threshold=thr or 0,
                                 opponent=opponent, muzero_player=int(mzp))
                left -= m
            actor.flush(on_game=lambda e, gh: finished.append(gh))
        assert len(finished) == 1, (run, len(finished))
        check_against_g6(fx, run, finished[0], A, config, near_ties)
        state = actor.engine.get_rng_state(0)
        assert int(state[2]) == int(fx[f"run{run}_rng_pos_end"]), run
        np.random.set_state(state)
        assert int(np.random.randint(0, 2**31 - 1)) == int(fx[f"run{run}_rng_next_word"]), run
        actor.close()


# ---- many envs against the host plugins -----------------------------------------------------------------------------
def host_games(sp, weights, game, config, seed, E, opponent, mzp, n_moves, temperature=0, threshold=None):
    finished = [[] for _ in range(E)]
    actor = sp.BatchedSelfPlay({"weights": weights}, games(game).Game, config, seed, E, use_graph=False)
    for _ in range(n_moves):
        actor.step(temperature, threshold, on_game=lambda e, gh: finished[e].append(gh), opponent=opponent, muzero_player=mzp)
    actor.close()
    return finished


def assert_same_games(got, want, where):
    assert [len(g) for g in got] == [len(g) for g in want], where
    for e, (mine, theirs) in enumerate(zip(got, want)):
        for a, b in zip(mine, theirs):
            assert a.action_history == b.action_history, (where, e)
            assert a.reward_history == b.reward_history and a.to_play_history == b.to_play_history, (where, e)
            assert [v is None for v in a.root_values] == [v is None for v in b.root_values], (where, e)
            assert np.array_equal(np.array(a.child_visits, dtype=float), np.array(b.child_visits, dtype=float)), (where, e)
            np.testing.assert_allclose([v for v in a.root_values if v is not None], [v for v in b.root_values if v is not None],
                                       rtol=0, atol=RESNET_TOL["value_tol"])
            assert np.array_equal(np.array(a.observation_history), np.array(b.observation_history, dtype=np.float32)), (where, e)


@pytest.mark.parametrize("game,fc,E", [("tictactoe", False, 3), ("tictactoe", False, 64), ("tictactoe", True, 64),
                                       ("connect4", False, 3), ("connect4", True, 64)])
@pytest.mark.parametrize("opponent,mzp", [("expert", 1), ("random", 0)])
def test_device_actors_play_the_host_actors_opponent_games(sp, models_mod, game, fc, E, opponent, mzp):
    """E device envs against an expert (MuZero second: the opponent opens every game) and a random opponent, fully-
    connected (fused whole-move search) and residual (lock-step) networks: DeviceSelfPlay in batches of 1, 4 and 9 moves
    -- games end and restart inside them -- and PipelinedDeviceSelfPlay (2 groups; with and without hipGraph) file, env
    by env, the games BatchedSelfPlay files with the host Game plugins."""
    config = game_config(game, fc)
    _, weights = synthetic_model(models_mod, config, "cpu")
    sizes = [1, 4, 9, 4, 9] if game == "connect4" else [1, 4, 9, 4]
    n_moves = sum(sizes)
    want = host_games(sp, weights, game, config, 40, E, opponent, mzp, n_moves)
    assert sum(len(g) for g in want) >= E                       # games did end (and restart) inside the batches
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 40, E)
    for m in sizes:
        played = actor.play_moves(m, 0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0, opponent=opponent,
                                  muzero_player=mzp)
        assert (played == m).all()                              # opponent plies keep an env live in the batch
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    actor.close()
    assert_same_games(got, want, f"{game} {opponent} batches")
    if E % 2 == 0:
        for use_graph in (True, False):
            got = [[] for _ in range(E)]
            actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 40, E, groups=2, use_graph=use_graph)
            for m in sizes:
                actor.play_moves(m, 0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0, opponent=opponent,
                                 muzero_player=mzp)
            actor.flush(on_game=lambda e, gh: got[e].append(gh))
            actor.close()
            assert_same_games(got, want, f"{game} {opponent} pipelined graph={use_graph}")
        # move by move with the opponent given to step() itself (nothing set on the actor beforehand)
        got = [[] for _ in range(E)]
        actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 40, E, groups=2)
        for _ in range(n_moves):
            actor.step(0, None, on_game=lambda e, gh: got[e].append(gh), opponent=opponent, muzero_player=mzp)
        assert all(a.envs.opponent == (opponent, mzp) for a in actor.actors)
        assert 0 < actor.searched_moves < actor.moves_played == n_moves * E
        assert_same_games(got, want, f"{game} {opponent} pipelined steps")
        actor.step(0, None, prefetch=False)                     # and back: a step without an opponent is self-play
        assert all(a.envs.opponent == ("self", 0) for a in actor.actors)
        actor.close()
    else:
        # move by move: every step a one-move batch; then back to self-play on the same actor
        got = [[] for _ in range(E)]
        actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 40, E)
        for _ in range(n_moves):
            actor.step(0, None, on_game=lambda e, gh: got[e].append(gh), opponent=opponent, muzero_player=mzp)
        assert_same_games(got, want, f"{game} {opponent} steps")
        actor.step(0, None)
        assert actor.envs.opponent == ("self", 0)
        actor.close()


def test_temperature_threshold_counts_opponent_plies(sp, models_mod):
    """play_game's rule len(action_history) < threshold sees the opponent's plies: batches at T = 1 with threshold 3
    against a random opponent equal BatchedSelfPlay's games."""
    config = game_config("tictactoe")
    _, weights = synthetic_model(models_mod, config, "cpu")
    E, sizes = 16, [3, 5, 9, 2]
    for mzp in (0, 1):
        want = host_games(sp, weights, "tictactoe", config, 7, E, "random", mzp, sum(sizes), temperature=1.0, threshold=3)
        got = [[] for _ in range(E)]
        actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 7, E)
        for m in sizes:
            actor.play_moves(m, 1.0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=3, opponent="random",
                             muzero_player=mzp)
        actor.flush(on_game=lambda e, gh: got[e].append(gh))
        actor.close()
        assert_same_games(got, want, f"threshold mzp={mzp}")


def test_step_against_an_opponent_names_what_rules_it_out(sp, models_mod):
    config = game_config("tictactoe")
    _, weights = synthetic_model(models_mod, config, "cpu")
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 2)
    with pytest.raises(NotImplementedError, match="temperature 0, inf or 1/k"):
        actor.step(0.3, None, opponent="expert", muzero_player=0)
    with pytest.raises(NotImplementedError, match='"human": use SelfPlay'):
        actor.step(0, None, opponent="human", muzero_player=0)
    actor.config.root_dirichlet_alpha = 1.5
    with pytest.raises(NotImplementedError, match="root_dirichlet_alpha"):
        actor.step(0, None, opponent="expert", muzero_player=0)
    actor.close()


# ---- the training loop's test mode and the public entry -----------------------------------------------------------------
class Storage:
    def __init__(self, weights):
        self.info = {"training_step": 0, "terminate": False, "weights": weights}
        self.metrics = []

    def get_info(self, key):
        return self.info[key]

    def set_info(self, keys, values=None):
        self.metrics.append(dict(keys))
        if "muzero_reward" in keys:
            self.info["training_step"] += 1                 # (one test game per "training step": ends the loop)


@pytest.mark.parametrize("kind", ["device", "pipelined"])
def test_continuous_self_play_test_mode_on_device_actors(sp, models_mod, kind):
    """ManyEnvLoop.continuous_self_play(test_mode=True) with moves_per_pass (the move-batch path) on the device actors
    reports the metric dictionaries the SelfPlay facade reports for the same seed."""
    ttt = games("tictactoe")
    _, weights = synthetic_model(models_mod, ttt.MuZeroConfig(), "cpu")
    stores = []
    for who in ("facade", kind):
        cfg = ttt.MuZeroConfig()
        cfg.opponent, cfg.muzero_player, cfg.training_steps = "expert", 0, 2
        store = Storage(weights)
        if who == "facade":
            sp.SelfPlay({"weights": weights}, ttt.Game, cfg, 30).continuous_self_play(store, None, True)
            stores.append(store.metrics[:4])
            continue
        if who == "device":
            actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", cfg, 30, 1)
        else:
            actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", cfg, 30, 2, groups=2)
        actor.continuous_self_play(store, None, True, moves_per_pass=3)
        # env 0 is the facade's worker (seed 30): its games come first among each pass's
        stores.append(store.metrics)
    facade, many = stores
    assert len(facade) == 4 and {"muzero_reward", "opponent_reward"} <= set(facade[1])
    if kind == "device":
        assert len(many) >= 4
        for a, b in zip(facade, many[:4]):
            assert set(a) == set(b)
            for k in a:
                assert a[k] == pytest.approx(b[k], abs=RESNET_TOL["value_tol"]), k
    else:
        # (two envs: env 0 is the facade's worker; its first game's metrics are among those reported)
        assert len(many) >= 4 and all(set(a) == set(b) for a, b in zip(facade, many[:4]))
        assert any(set(m) == set(facade[0]) and all(m[k] == pytest.approx(v, abs=RESNET_TOL["value_tol"]) for k, v in facade[0].items())
                   for m in many)


def test_evaluate_equals_consecutive_play_games_and_counts_add_up(sp, models_mod):
    ttt = games("tictactoe")
    config = ttt.MuZeroConfig()
    _, weights = synthetic_model(models_mod, config, "cpu")
    for opponent, mzp in (("expert", 0), ("random", 1)):
        single = sp.SelfPlay({"weights": weights}, ttt.Game, config, 11)
        ghs = [single.play_game(0, 0, False, opponent, mzp) for _ in range(3)]
        single.close_game()
        mine = [sum(r for i, r in enumerate(g.reward_history) if g.to_play_history[i - 1] == mzp) for g in ghs]
        theirs = [sum(r for i, r in enumerate(g.reward_history) if g.to_play_history[i - 1] != mzp) for g in ghs]
        out = sp.evaluate({"weights": weights}, "tictactoe", config, 3, opponent=opponent, muzero_player=mzp, num_envs=1,
                          seed=11)
        assert out["games"] == 3 and out["result"] == pytest.approx(np.mean(mine)) and out["muzero_reward"] == out["result"]
        assert out["opponent_reward"] == pytest.approx(np.mean(theirs))
        assert out["mean_episode_length"] == pytest.approx(np.mean([len(g.action_history) - 1 for g in ghs]))
        assert (out["wins"], out["losses"]) == (sum(m > t for m, t in zip(mine, theirs)), sum(m < t for m, t in zip(mine, theirs)))
    cfg = ttt.MuZeroConfig()
    cfg.opponent, cfg.muzero_player = "expert", 1
    out = sp.evaluate({"weights": weights}, "tictactoe", cfg, 200, num_envs=64, seed=5)          # None: the config's values
    assert out["games"] == 200 and out["wins"] + out["draws"] + out["losses"] == 200
    assert (out["opponent"], out["muzero_player"]) == ("expert", 1)
    assert 5 <= out["mean_episode_length"] <= 9 and 0 < out["searched_moves"] < out["env_moves"]
    explicit = sp.evaluate({"weights": weights}, "tictactoe", cfg, 200, opponent="expert", muzero_player=0, num_envs=64, seed=5)
    assert explicit["muzero_player"] == 0                       # an explicit 0 is 0 (the reference falls back to the config)
    solo = sp.evaluate({"weights": weights}, "tictactoe", cfg, 10, opponent="self", num_envs=4, seed=5)
    assert solo["games"] == 10 and solo["searched_moves"] == solo["env_moves"]
