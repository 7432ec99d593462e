"""Paired mode of the device actors (set_opponent(paired=True): the opponent replies inside MuZero's move) plays the
games the sit-out mode plays: same seed, same network, games compared env by env; the engine's RNG mirrors compared where
both actors stand at the same ply of the same game; evaluate(paired=True) against evaluate(paired=False)."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import synthetic_model

pytestmark = pytest.mark.gpu

E, BATCH, GAMES = 16, 4, 3


@pytest.fixture(scope="module")
def sp(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.self_play")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def game_config(name, fc=False, simulations=None):
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{name}").MuZeroConfig()
    if fc:
        config.network, config.encoding_size = "fullyconnected", 16
        config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
        config.num_simulations = min(config.num_simulations, 25)       # (the fused kernel keeps the trees in LDS)
    if simulations:
        config.num_simulations = simulations
    return config


def rng_state(actor, e):
    if hasattr(actor, "actors"):
        return actor.actors[e // actor.per_group].engine.get_rng_state(e % actor.per_group)
    return actor.engine.get_rng_state(e)


def play(sp, weights, game, config, opponent, mzp, paired, batches, singles=0, temperature=0, groups=1):
    """`batches` batches of BATCH moves, then `singles` one-move batches.  Returns (finished games per env, plies per env,
    {(env, plies played): RNG state} at every batch boundary)."""
    if groups > 1:
        actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 40, E, groups=groups)
    else:
        actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 40, E)
    actor.set_opponent(opponent, mzp, paired=paired)
    finished, plies, states = [[] for _ in range(E)], np.zeros(E, dtype=np.int64), {}
    collect = lambda e, gh: finished[e].append(gh)
    for n in [BATCH] * batches + [1] * singles:
        plies += actor.play_moves(n, temperature, on_game=collect, temperature_threshold=0)
        actor.flush(on_game=collect)
        for e in range(E):
            states[(e, int(plies[e]))] = rng_state(actor, e)
    searched, played = actor.searched_moves, actor.moves_played
    actor.close()
    return finished, plies, states, searched, played


def assert_same_games(got, want, where):
    """Env by env the first GAMES finished games: actions, rewards, to_play, observations, child_visits, root values."""
    for e, (mine, theirs) in enumerate(zip(got, want)):
        assert len(mine) >= GAMES and len(theirs) >= GAMES, (where, e, len(mine), len(theirs))
        for a, b in zip(mine[:GAMES], theirs[:GAMES]):
            assert a.action_history == b.action_history, (where, e)
            assert a.reward_history == b.reward_history and a.to_play_history == b.to_play_history, (where, e)
            assert np.array_equal(np.array(a.observation_history), np.array(b.observation_history)), (where, e)
            assert a.child_visits == b.child_visits, (where, e)
            assert a.root_values == b.root_values, (where, e)          # (None on the opponent's plies)
            assert any(v is None for v in a.root_values) and any(v is not None for v in a.root_values)


def compare_modes(sp, models_mod, game, config, opponent, mzp, temperature=0, groups=1):
    _, weights = synthetic_model(models_mod, config, "cpu")
    # a game is at most `longest` plies and a paired move plays at least one: GAMES games are over after GAMES * longest
    # moves at the latest, which tic-tac-toe plays.  Connect four's paired actor, which mostly plays two plies a move,
    # plays 20 batches: they finish GAMES games in every env of this seeded case (asserted below; the games are
    # deterministic).  The sit-out actor then plays batches up to the fewest plies a paired env played and goes on move
    # by move to the most: it finishes the same games and has a batch boundary at every paired env's ply count.
    longest = 9 if game == "tictactoe" else 42
    pair_batches = -(-GAMES * longest // BATCH) if game == "tictactoe" else 20
    got, plies, states, searched, played = play(sp, weights, game, config, opponent, mzp, True, pair_batches,
                                                temperature=temperature, groups=groups)
    sit_batches = int(plies.min()) // BATCH
    want, sit_plies, sit_states, sit_searched, sit_played = play(sp, weights, game, config, opponent, mzp, False, sit_batches,
                                                                 singles=int(plies.max()) - sit_batches * BATCH,
                                                                 temperature=temperature, groups=groups)
    where = f"{game} {opponent} mzp={mzp} T={temperature} groups={groups}"
    assert_same_games(got, want, where)
    # counters: moves_played in plies, searched_moves in searches (every move of the paired actor searched every env)
    assert played == int(plies.sum()) and searched == pair_batches * BATCH * E, where
    assert sit_played == int(sit_plies.sum()) and 0 < sit_searched < sit_played, where
    # the streams: where the paired actor stands after as many plies as the sit-out actor stood at a batch boundary, both
    # stand in the same position of the same game with no ply in flight, and the RNG mirrors must be equal
    for e in range(E):
        mine, theirs = states[(e, int(plies[e]))], sit_states[(e, int(plies[e]))]
        assert mine[2] == theirs[2] and np.array_equal(mine[1], theirs[1]), (where, e)


@pytest.mark.parametrize("mzp", [0, 1])
@pytest.mark.parametrize("fc", [True, False], ids=["fused-fc", "lockstep-resnet"])
def test_paired_games_equal_sit_out_games_tictactoe_expert(sp, models_mod, fc, mzp):
    compare_modes(sp, models_mod, "tictactoe", game_config("tictactoe", fc, None if fc else 10), "expert", mzp)


def test_paired_games_equal_sit_out_games_connect4_random(sp, models_mod):
    compare_modes(sp, models_mod, "connect4", game_config("connect4", simulations=10), "random", 0)


def test_paired_games_equal_sit_out_games_pipelined(sp, models_mod):
    compare_modes(sp, models_mod, "tictactoe", game_config("tictactoe", simulations=10), "expert", 1, groups=2)


def test_paired_games_equal_sit_out_games_sampled_at_temperature_one(sp, models_mod):
    """T = 1 is sampled on the device without set_device_temperatures: the sampler's draws come from the env's stream
    between the opponent's, so equal games pin the order of the draws."""
    compare_modes(sp, models_mod, "tictactoe", game_config("tictactoe", simulations=10), "expert", 0, temperature=1.0)


def test_paired_mode_refusals(sp, models_mod):
    config = game_config("tictactoe", simulations=10)
    _, weights = synthetic_model(models_mod, config, "cpu")
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 4)
    actor.set_opponent("expert", 0, paired=True)
    with pytest.raises(NotImplementedError, match="temperature_threshold"):
        actor.play_moves(2, 1.0, temperature_threshold=3)
    with pytest.raises(NotImplementedError, match=r"step\(\) in paired mode"):
        actor.step(0, 0)
    assert (actor.play_moves(2, 0, temperature_threshold=0) >= 2).all()          # (the refusals left the actor usable)
    actor.close()
    pipelined = sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 4, groups=2)
    pipelined.set_opponent("expert", 0, paired=True)
    with pytest.raises(NotImplementedError, match=r"step\(\) in paired mode"):
        pipelined.step(0, 0)
    pipelined.close()
    stacked = game_config("tictactoe", simulations=10)
    stacked.stacked_observations = 2
    _, weights = synthetic_model(models_mod, stacked, "cpu")
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", stacked, 0, 4)
    actor.set_opponent("expert", 0, paired=True)
    with pytest.raises(NotImplementedError, match="stacked_observations"):
        actor.play_moves(2, 0, temperature_threshold=0)
    actor.close()


@pytest.mark.parametrize("mzp", [0, 1])
def test_evaluate_paired_equals_evaluate_sit_out(sp, models_mod, mzp):
    """Which games count is decided per env and per ply, so both modes select the same 64 games."""
    config = game_config("tictactoe", simulations=10)
    _, weights = synthetic_model(models_mod, config, "cpu")
    out = {paired: sp.evaluate({"weights": weights}, "tictactoe", config, 64, opponent="expert", muzero_player=mzp,
                               num_envs=16, seed=3, paired=paired) for paired in (False, True)}
    for key in ("result", "muzero_reward", "opponent_reward", "mean_episode_length", "wins", "draws", "losses", "games"):
        assert out[True][key] == out[False][key], key
    assert out[True]["games"] == 64 and out[True]["paired"] and not out[False]["paired"]
