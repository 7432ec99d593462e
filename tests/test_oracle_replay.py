"""Oracle of the replay-target row against the reference's own ReplayBuffer: sampled batches (fixtures
G12), reanalysed CartPole games (G13), and every position of the edge-case games of G17 (two-player bootstraps, games
past 256 plies and of exactly max_moves plies, deep stacks, reanalysed two-player games)."""
import importlib
import os
import sys

import numpy as np
import pytest

from parity_helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

NAMES = ["cartpole", "tictactoe", "tictactoe_stacked", "cartpole_uniform"]
EDGE_NAMES = ["tictactoe_td3", "connect4_td5", "cartpole_long", "cartpole_alpha1"]
KINDS = {int: 0, float: 1, np.float32: 2, np.float64: 3}      # result types as fixture G17 codes them


def games_of(fx, ro):
    games = []
    for g, n in enumerate(fx["lengths"]):
        games.append(ro.Game(fx["observations"][g, : n + 1], fx["actions"][g, : n + 1], fx["rewards"][g, : n + 1],
                             fx["to_play"][g, : n + 1], fx["child_visits"][g, :n], fx["root_values"][g, :n]))
    return games


def cfg_of(fx):
    return dict(batch_size=int(fx["batch_size"]), PER=bool(fx["PER"]), td_steps=int(fx["td_steps"]),
                discount=float(fx["cfg_discount"]), num_unroll_steps=int(fx["num_unroll_steps"]),
                action_space=list(range(int(fx["cfg_A"]))), stacked_observations=int(fx["stacked_observations"]))


@pytest.mark.parametrize("name", NAMES)
def test_replay_oracle_matches_reference(oracle, name):
    ro = importlib.import_module("replay_oracle")
    fx = load_golden(f"g12_replay_{name}")
    games, cfg = games_of(fx, ro), cfg_of(fx)
    if cfg["PER"]:
        for g, game in enumerate(games):
            pri = ro.initial_priorities(game, cfg["td_steps"], cfg["discount"], float(fx["PER_alpha"]))
            assert np.array_equal(pri, fx["priorities"][g, : len(pri)]), g       # float32, bit for bit
            assert game.game_priority == fx["game_priority"][g]
    rng = oracle.Rng(int(fx["seed"]))
    out = ro.get_batch(games, cfg, rng)
    assert np.array_equal(np.array(out["index"]), fx["index_batch"])
    assert np.array_equal(np.array(out["action"]), fx["action_batch"])
    assert np.array_equal(np.array(out["value"], dtype=np.float64), fx["value_batch"])
    assert np.array_equal(np.array(out["reward"], dtype=np.float64), fx["reward_batch"])
    assert np.array_equal(np.array(out["policy"], dtype=np.float64), fx["policy_batch"])
    assert np.array_equal(np.array(out["gradient_scale"], dtype=np.float64), fx["gradient_scale_batch"])
    assert np.array_equal(np.array(out["observation"], dtype=np.float32), fx["observation_batch"])
    if cfg["PER"]:
        assert np.array_equal(out["weight"], fx["weight_batch"])


def test_replay_oracle_with_reanalysed_values(oracle):
    ro = importlib.import_module("replay_oracle")
    fx = load_golden("g13_reanalyse_cartpole")
    games = games_of(fx, ro)
    for g, game in enumerate(games):
        game.reanalysed = fx["reanalysed"][g, : len(game.root_values)].copy()
    rng = oracle.Rng(int(fx["seed"]))
    for i, (g, pos) in enumerate(fx["pairs"]):
        v, r, p, a = ro.make_target(games[g], int(pos), int(fx["td_steps"]), float(fx["cfg_discount"]),
                                    int(fx["num_unroll_steps"]), list(range(int(fx["cfg_A"]))), rng)
        assert np.array_equal(np.array([float(x) for x in v]), fx["value_targets"][i]), (g, pos)
        assert np.array_equal(np.array(r, dtype=np.float64), fx["reward_targets"][i])
        assert np.array_equal(np.array(p, dtype=np.float64), fx["policy_targets"][i])
        assert np.array_equal(np.array(a), fx["action_targets"][i])


def edge_discount(fx):
    """config.discount with the reference's type: the board games have the int 1, CartPole a float."""
    return int(fx["cfg_discount"]) if int(fx["discount_is_int"]) else float(fx["cfg_discount"])


def install_reanalysed(fx, games):
    for g in np.flatnonzero(fx["has_reanalysed"]):
        games[g].reanalysed = fx["reanalysed"][g, : len(games[g].root_values)].copy()


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_replay_oracle_at_every_position_of_the_edge_games(oracle, name):
    """Fixture G17: priorities, compute_target_value (value and result type), make_target and the stacked observation
    of EVERY position, before and after half of the games carry float32 reanalysed values.  The float32 results are a
    property of NumPy >= 2 promotion (a numpy float32 scalar times / plus a Python float stays float32); the fixture
    names the NumPy that recorded it."""
    ro = importlib.import_module("replay_oracle")
    fx = load_golden(f"g17_replay_edges_{name}")
    assert int(str(fx["numpy_version"]).split(".")[0]) >= 2 and int(np.__version__.split(".")[0]) >= 2
    games = games_of(fx, ro)
    td, unroll, discount = int(fx["td_steps"]), int(fx["num_unroll_steps"]), edge_discount(fx)
    action_space, stacked = list(range(int(fx["cfg_A"]))), int(fx["stacked_observations"])
    lengths = fx["lengths"]
    assert 1 in lengths and int(fx["max_moves"]) in lengths and fx["observations"].shape[1] == int(fx["max_moves"]) + 1
    for g, game in enumerate(games):
        pri = ro.initial_priorities(game, td, discount, float(fx["PER_alpha"]))
        assert np.array_equal(pri, fx["priorities"][g, : len(pri)]), g       # float32, bit for bit
        assert game.game_priority == fx["game_priority"][g]
        assert not fx["priorities"][g, len(pri):].any()
    pairs = fx["pairs"]
    assert len(pairs) == lengths.sum()
    for i, (g, pos) in enumerate(pairs):
        assert np.array_equal(ro.stacked_observations(games[g], int(pos), stacked), fx["stacked"][i]), (g, pos)
    for tag in ("before", "after"):
        if tag == "after":
            install_reanalysed(fx, games)
        rng = oracle.Rng(int(fx[f"seed_{tag}"]))
        draws = []
        for i, (g, pos) in enumerate(pairs):
            g, pos = int(g), int(pos)
            target = ro.compute_target_value(games[g], pos, td, discount)
            assert float(target) == fx[f"target_value_{tag}"][i], (tag, g, pos)
            assert KINDS[type(target)] == fx[f"target_kind_{tag}"][i], (tag, g, pos, type(target))
            v, r, p, a = ro.make_target(games[g], pos, td, discount, unroll, action_space, rng)
            assert np.array_equal(np.array([float(x) for x in v]), fx[f"value_targets_{tag}"][i]), (tag, g, pos)
            assert [KINDS[type(x)] for x in v] == fx[f"value_kind_{tag}"][i].tolist(), (tag, g, pos)
            assert np.array_equal(np.array(r, dtype=np.float64), fx["reward_targets"][i]), (tag, g, pos)
            assert np.array_equal(np.array(p, dtype=np.float64), fx["policy_targets"][i]), (tag, g, pos)
            assert np.array_equal(np.array(a), fx[f"action_targets_{tag}"][i]), (tag, g, pos)
            draws.extend(a[u] for u in range(unroll + 1) if pos + u > lengths[g])
        assert np.array_equal(np.array(draws), fx[f"absorbing_draws_{tag}"])
    # the branches this fixture exists for are in it
    boot = np.array([pos + td < lengths[g] for g, pos in pairs])
    assert boot.any() and (~boot).any()
    f32 = fx["target_kind_after"] == KINDS[np.float32]
    assert np.array_equal(f32, boot & fx["has_reanalysed"][pairs[:, 0]]) and (fx["target_kind_before"] == KINDS[float]).all()
    if int(fx["cfg_players"]) == 2:
        flipped = [games[g].to_play[pos + td] != games[g].to_play[pos] for (g, pos), b in zip(pairs, boot) if b]
        assert any(flipped)
