"""What finished games report, on the card (csrc/game_outcomes.h; include/mzreplay.h mzreplay_game_outcomes and the filer's
outcome list; self_play.GameOutcomes; training_loop.TrainingLoop).

* mzreplay_game_outcomes on a store that holds every game of tests/game_outcomes_reference.py (max_moves 512, a 1 x 1 x 4
  observation), each slot first filled to the brim with NaN so that a read past a game's end poisons the result: equal
  to the library's host entry bit for bit, twice.
* The filer's outcomes against a host twin: the same weights and seeds played through on_games -> save_games, every
  PackedGames row put through the host entry.  Outcome for outcome, in on_games order, ids as the store gave them; the
  store's own game_outcomes of the stored games agrees; the store is the host twin's (test_gpu_replay_filer
  assert_same_stores), and the store of a third actor that files with outcomes off is byte-equal too.
* A refused batch reports no outcomes; the refusals that need a store.
* TrainingLoop: CartPole rows with device filing, with the host twin and a second run; TicTacToe with the residual network
  and an evaluation."""
import ctypes
import importlib
import math
import types

import numpy as np
import pytest
import torch

import game_outcomes_reference as ref
from parity_helpers import synthetic_model
from replay_filer_cases import file_moves
from test_gpu_replay_filer import START, assert_same_stores, cartpole_weights, close_all, games, tictactoe_fc

pytestmark = pytest.mark.gpu
FIELDS = ("total_reward", "reward_of_player", "value_sum", "value_count")


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return types.SimpleNamespace(rb=importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
                                 sp=importlib.import_module("muzero-hypermodel_amd.self_play"),
                                 models=importlib.import_module("muzero-hypermodel_amd.models"),
                                 native=importlib.import_module("muzero-hypermodel_amd._native"),
                                 loop=importlib.import_module("muzero-hypermodel_amd.training_loop"))


def same_records(got, want, what):
    """Two GAME_OUTCOME_DTYPE arrays, bit for bit (a NaN sum equals a NaN sum)."""
    assert len(got) == len(want), what
    for key in FIELDS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if a.dtype == np.float64:
            same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        assert same.all(), f"{what}: {key} of game {int(np.flatnonzero(~same.reshape(len(got), -1).all(axis=1))[0])}"


def as_records(native, outcomes):
    """A self_play.GameOutcomes as a GAME_OUTCOME_DTYPE array."""
    out = np.zeros(len(outcomes), dtype=native.GAME_OUTCOME_DTYPE)
    for key in FIELDS:
        out[key] = getattr(outcomes, key)
    return out


def host_records(native, batch):
    """The host entry on every row of a PackedGames."""
    out = np.zeros(len(batch), dtype=native.GAME_OUTCOME_DTYPE)
    for i, n in enumerate(batch.length):
        n = int(n)
        out[i] = native.outcomes_reference(np.asarray(batch.rewards[i, : n + 1], dtype=np.float64), batch.to_play[i, : n + 1],
                                           batch.root_values[i, :n])
    return out


# ---- stored games ------------------------------------------------------------------------------------------------------------
def test_stored_games_between_nan_guard_bands(mods):
    cases = ref.make_cases() + ref.directed_cases()
    G, L = len(cases), ref.MAX_MOVES
    config = games("cartpole").MuZeroConfig()               # a 1 x 1 x 4 observation, two actions
    config.max_moves, config.replay_buffer_size, config.PER = L, G, False
    assert tuple(config.observation_shape) == (1, 1, 4)
    store = mods.rb.ReplayBuffer(START, {}, config)
    rs = np.random.RandomState(3)

    def packed(lengths, rewards, to_play, values):
        return mods.sp.PackedGames(env_index=np.arange(G, dtype=np.int32), length=np.asarray(lengths, dtype=np.int32),
                                   observations=rs.standard_normal((G, L + 1, 1, 1, 4)).astype(np.float32),
                                   actions=np.zeros((G, L + 1), dtype=np.int32), rewards=rewards, to_play=to_play,
                                   child_visits=np.full((G, L, 2), 0.5), root_values=values)
    # the guard bands: every slot whole, NaN rewards and values and player 1 throughout
    store.save_games(packed([L] * G, np.full((G, L + 1), np.nan), np.ones((G, L + 1), dtype=np.int32), np.full((G, L), np.nan)))
    rewards, to_play, values = np.full((G, L + 1), np.nan), np.ones((G, L + 1), dtype=np.int32), np.full((G, L), np.nan)
    for g, case in enumerate(cases):
        rewards[g, : case.n + 1], to_play[g, : case.n + 1], values[g, : case.n] = case.rewards, case.to_play, case.root_values
    store.save_games(packed([case.n for case in cases], rewards, to_play, values))   # ids G .. 2G - 1: the same slots
    assert list(store.buffer) == list(range(G, 2 * G))
    want = np.array([mods.native.outcomes_reference(c.rewards, c.to_play, c.root_values) for c in cases],
                    dtype=mods.native.GAME_OUTCOME_DTYPE)
    assert np.isnan(want["value_sum"]).sum() == len(ref.LENGTHS)            # (the NaN cases, and no other)
    for turn in range(2):
        got = store.game_outcomes(range(G, 2 * G))
        assert got.length.tolist() == [c.n for c in cases] and got.game_id.tolist() == list(range(G, 2 * G))
        assert (got.env_index == -1).all()
        same_records(as_records(mods.native, got), want, f"stored games, turn {turn}")
    for case, mean in zip(cases, got.mean_value):                           # and numpy.mean itself
        assert ref.same_bits(mean, ref.restate(case)["mean_value"]), case.name
    some = store.game_outcomes([G + 5, G + 5, 2 * G - 1])                     # any order, repeats
    same_records(as_records(mods.native, some), want[[5, 5, G - 1]], "picked games")
    with pytest.raises(KeyError):
        store.game_outcomes([0])
    # the refusals that need a store
    lib, out = mods.native.load(), np.zeros(2, dtype=mods.native.GAME_OUTCOME_DTYPE)
    for bad in (-1, G):
        slots = np.array([0, bad], dtype=np.int32)
        assert lib.mzreplay_game_outcomes(store._h, 2, mods.native.ptr(slots, mods.native.c_i32_p), out.ctypes.data, None) == -1
        assert b"slot out of range" in lib.mzreplay_last_error(store._h)
    assert lib.mzreplay_game_outcomes(store._h, -1, mods.native.ptr(slots, mods.native.c_i32_p), out.ctypes.data, None) == -1
    assert lib.mzreplay_game_outcomes(store._h, 1, None, out.ctypes.data, None) == -1
    assert lib.mzreplay_game_outcomes(store._h, 0, mods.native.ptr(slots, mods.native.c_i32_p), out.ctypes.data, None) == 0
    store.close()


# ---- the filer against the host twin ---------------------------------------------------------------------------------------------
def outcome_twins(mods, make_actor, config, sizes, plain_twin=False, play=None, want_overflow=False):
    """Actor A through on_games -> save_games into store A (the host entry on every row), actor B with
    file_to(store B, outcomes=True), optionally actor C with file_to(store C); the same play_moves sizes and a flush."""
    play = play or (lambda actor, n, on_games: actor.play_moves(n, 1.0, on_games=on_games))
    stores = [mods.rb.ReplayBuffer(START, {}, config) for _ in range(3 if plain_twin else 2)]
    actors = [make_actor() for _ in stores]
    actors[1].file_to(stores[1], outcomes=True)
    if plain_twin:
        actors[2].file_to(stores[2])
        with pytest.raises(RuntimeError, match="outcomes=True"):
            actors[2].take_outcomes()
    with pytest.raises(RuntimeError, match="outcomes=True"):
        actors[0].take_outcomes()                           # (host rows: nothing is filed on the device)
    want_env, want_len, want, filed, got = [], [], [], [], []

    def host_games(batch):
        want_env.append(np.asarray(batch.env_index).copy())
        want_len.append(np.asarray(batch.length).copy())
        want.append(host_records(mods.native, batch))
        stores[0].save_games(batch)

    def take():
        outcomes = actors[1].take_outcomes()
        assert len(outcomes) == sum(len(f) for f in filed) - sum(len(o) for o in got)
        got.append(outcomes)
    for n in sizes:
        play(actors[0], n, host_games)
        play(actors[1], n, filed.append)
        take()
        if plain_twin:
            play(actors[2], n, None)
    actors[0].flush(on_games=host_games)
    actors[1].flush(on_games=filed.append)
    take()
    if plain_twin:
        actors[2].flush()
    assert len(actors[1].take_outcomes()) == 0               # taken once
    outcomes = mods.sp.GameOutcomes.concatenate(got)
    assert len(outcomes) == actors[1].games_finished == sum(len(f) for f in filed) > 0
    assert np.array_equal(outcomes.env_index, np.concatenate(want_env))
    assert np.array_equal(outcomes.length, np.concatenate(want_len))
    assert np.array_equal(outcomes.game_id, np.concatenate([f.game_id for f in filed]))
    assert np.array_equal(outcomes.game_id, np.arange(len(outcomes)))
    same_records(as_records(mods.native, outcomes), np.concatenate(want), "filed games")
    if want_overflow:
        assert any(len(f) > stores[1].capacity for f in filed), "no call finished more games than the store has slots"
    # the store agrees about the games it still holds, and is the host twin's
    kept = list(stores[1].buffer)
    same_records(as_records(mods.native, stores[1].game_outcomes(kept)), as_records(mods.native, outcomes)[kept], "stored games")
    assert_same_stores(stores[0], stores[1], "host twin", False)
    if plain_twin:
        assert_same_stores(stores[2], stores[1], "outcomes off", False)
    return outcomes, stores, actors


def test_cartpole_fused_batches(mods, pkg):
    """64 envs, 3 batches of 20 moves, the fused search; with the twin that files with outcomes off."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 30, 3, 400
    outcomes, stores, actors = outcome_twins(mods, lambda: mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 0, 64),
                                             config, (20, 20, 20), plain_twin=True)
    assert np.array_equal(outcomes.total_reward, outcomes.length.astype(np.float64))   # CartPole pays 1 per move
    assert np.array_equal(outcomes.reward_of_player[:, 0], outcomes.total_reward) and not outcomes.reward_of_player[:, 1].any()
    assert (outcomes.value_count > 0).all() and np.isfinite(outcomes.mean_value).all()
    close_all(*actors, *stores)


def test_tictactoe_two_players_several_games_per_call(mods):
    """The fully-connected network, 32 envs, 18 moves a call: two players, several games per env and call."""
    config, weights = tictactoe_fc(mods.models)
    config.td_steps, config.replay_buffer_size = 4, 400
    outcomes, stores, actors = outcome_twins(mods, lambda: mods.sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 32),
                                             config, (18, 18), plain_twin=True)
    env = outcomes.env_index.tolist()
    assert len(env) > 2 * 32                                                  # several games per env and call
    assert outcomes.reward_of_player[:, 1].any() and outcomes.reward_of_player[:, 0].any()   # both players win games
    assert np.array_equal(outcomes.reward_of_player.sum(axis=1), outcomes.total_reward)      # (rewards are 0 or 1)
    close_all(*actors, *stores)


def test_tictactoe_residual_lockstep(mods):
    config = games("tictactoe").MuZeroConfig()
    config.blocks, config.channels, config.num_simulations = 1, 16, 10
    config.td_steps, config.replay_buffer_size, config.temperature_threshold = 4, 100, None
    _, weights = synthetic_model(mods.models, config, "cpu")
    outcomes, stores, actors = outcome_twins(mods, lambda: mods.sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 16),
                                             config, (9, 7))
    close_all(*actors, *stores)


def test_dropped_games_still_report(mods, pkg):
    """64 envs into 8 slots: a call finishes more games than the store has slots; every one of them reports."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 6, 2, 8
    outcomes, stores, actors = outcome_twins(mods, lambda: mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 0, 64),
                                             config, (8, 5, 9), want_overflow=True)
    assert len(stores[1].buffer) == 8 and len(outcomes) > 64
    assert np.array_equal(outcomes.total_reward, outcomes.length.astype(np.float64))
    close_all(*actors, *stores)


def test_two_pipelined_groups(mods):
    config, weights = tictactoe_fc(mods.models)
    config.td_steps, config.replay_buffer_size = 4, 200

    def play(actor, n, on_games):
        return actor.play_moves(n, 1.0, on_games=on_games, temperature_threshold=0)
    outcomes, stores, actors = outcome_twins(
        mods, lambda: mods.sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 16, groups=2), config,
        (5, 5, 5), play=play)
    assert {int(e) >= 8 for e in outcomes.env_index} == {False, True}            # global env indices, both groups
    close_all(*actors, *stores)


def test_two_actors_share_a_store(mods, pkg):
    """Two actors file into one store (shared=True), their calls alternating: each takes its own games' outcomes, which
    are those of its host twin, under the ids the store gave them."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 9, 3, 200
    store_a, store_b = mods.rb.ReplayBuffer(START, {}, config), mods.rb.ReplayBuffer(START, {}, config)
    shapes = ((0, 8), (100, 6))
    hosts = [mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, seed, E) for seed, E in shapes]
    filing = [mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, seed, E) for seed, E in shapes]
    filing[0].file_to(store_b, outcomes=True)
    filing[1].file_to(store_b, shared=True, outcomes=True)
    want, want_ids, got = [[], []], [[], []], [[], []]

    def host_games(k):
        def on_games(batch):
            first = store_a.num_played_games
            want[k].append(host_records(mods.native, batch))
            want_ids[k] += list(range(first, first + len(batch)))
            store_a.save_games(batch)
        return on_games
    for n in (7, 5, 9):
        for k in (0, 1):
            hosts[k].play_moves(n, 1.0, on_games=host_games(k))
            filing[k].play_moves(n, 1.0)
            got[k].append(filing[k].take_outcomes())
    for k in (1, 0):
        hosts[k].flush(on_games=host_games(k))
        filing[k].flush()
        got[k].append(filing[k].take_outcomes())
    for k in (0, 1):
        mine = mods.sp.GameOutcomes.concatenate(got[k])
        assert mine.game_id.tolist() == want_ids[k] and len(mine) == filing[k].games_finished > 0
        same_records(as_records(mods.native, mine), np.concatenate(want[k]), f"actor {k}")
    assert_same_stores(store_a, store_b, "two actors", False)
    close_all(*hosts, *filing, store_a, store_b)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_a_refused_batch_reports_nothing_and_the_switch_is_set_before_begin(mods):
    native = mods.native
    lib = native.load()
    config = games("tictactoe").MuZeroConfig()
    config.max_moves, config.replay_buffer_size = 4, 8
    store = mods.rb.ReplayBuffer(START, {}, config)
    E, M, A = 5, 2, 9
    dev = store.device
    obs_shape = tuple(int(v) for v in config.observation_shape)
    filer = store.attach_filer(E, outcomes=True)
    store.filer_begin(torch.zeros((E,) + obs_shape, device=dev), torch.zeros(E, dtype=torch.int32, device=dev))
    assert lib.mzreplay_filer_enable_outcomes(filer.handle, 0) == -1           # after begin the switch no longer moves
    assert b"before mzreplay_filer_begin" in lib.mzreplay_last_error(store._h)
    keep = dict(actions=torch.zeros((M, E), dtype=torch.int32, device=dev),
                visits=torch.ones((M, E, A), dtype=torch.int32, device=dev),
                rvs=torch.full((M, E), 2.5, dtype=torch.float64, device=dev),
                legal=torch.arange(A, dtype=torch.int32, device=dev).repeat(M, E, 1).contiguous(),
                num_legal=torch.full((M, E), A, dtype=torch.int32, device=dev),
                to_play=torch.tensor([[0] * E, [1] * E], dtype=torch.int32, device=dev),
                last=torch.zeros(E, dtype=torch.int32, device=dev),
                rewards=torch.tensor([[1.0] * E, [0.5] * E], dtype=torch.float32, device=dev),
                done=torch.tensor([[0] * E, [1] * E], dtype=torch.uint8, device=dev),
                obs_after=torch.ones((M, E) + obs_shape, device=dev), obs_next=torch.zeros((M, E) + obs_shape, device=dev))

    def check_good(first_id):
        env, length, ids = store.sync_filing()
        assert ids.tolist() == list(range(first_id, first_id + E)) and length.tolist() == [2] * E
        out = filer.take_outcomes()
        assert out.game_id.tolist() == ids.tolist() and out.env_index.tolist() == env.tolist()
        assert out.total_reward.tolist() == [1.5] * E
        assert out.reward_of_player.tolist() == [[1.0, 0.5]] * E              # move 0 by player 0, move 1 by player 1
        assert out.value_count.tolist() == [2] * E and out.value_sum.tolist() == [2 * 2.5 / 10] * E
    store.filer_file(file_moves(native, keep, M, 10, 2))
    check_good(0)
    keep["legal"][1, 3, 4] = A                                                 # a legal action of A: the batch is refused
    store.filer_file(file_moves(native, keep, M, 10, 2))
    with pytest.raises(RuntimeError, match="mzhist_file: a legal-action count outside"):
        store.sync_filing()
    assert len(filer.take_outcomes()) == 0
    keep["legal"][1, 3, 4] = 4
    store.filer_file(file_moves(native, keep, M, 10, 2))                       # the next good batch reports its own
    check_good(E)
    # a filer without the switch has no list to hand out
    plain = mods.rb.ReplayBuffer(START, {}, config)
    other = plain.attach_filer(E)
    n_out, out_p = ctypes.c_int32(), ctypes.c_void_p()
    assert lib.mzreplay_filer_sync_outcomes(other.handle, ctypes.byref(n_out), ctypes.byref(out_p)) == -1
    assert b"mzreplay_filer_enable_outcomes" in lib.mzreplay_last_error(plain._h)
    with pytest.raises(RuntimeError, match="outcomes=True"):
        other.take_outcomes()
    close_all(store, plain)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def strip(rows):
    return [{k: v for k, v in row.items() if k != "seconds"} for row in rows]


def cartpole_rows(mods, device_filing):
    config = mods.loop.game_config("cartpole", dict(training_steps=15))
    loop = mods.loop.TrainingLoop("cartpole", config, 64, 8, 5, seed=0, device_filing=device_filing)
    rows = loop.run(3)
    loop.close()
    return rows


@pytest.fixture(scope="module")
def first_rows(mods):
    return cartpole_rows(mods, True)


def test_the_loop_on_cartpole(first_rows):
    """64 envs, 3 iterations of 8 moves and 5 steps."""
    first = first_rows
    keys = {"iteration", "training_step", "num_played_games", "num_played_steps", "num_reanalysed_games", "lr", "temperature",
            "total_loss", "value_loss", "reward_loss", "policy_loss", "games_finished", "mean_total_reward", "max_total_reward",
            "mean_length", "mean_value", "mean_reward_player0", "mean_reward_player1", "eval", "seconds"}
    assert all(set(row) == keys for row in first)
    assert [row["training_step"] for row in first] == [0, 5, 10]               # (the first batch's games arrive with the second)
    assert first[-1]["games_finished"] > 0 and first[-1]["total_loss"] is not None
    assert all(math.isfinite(first[-1][k]) for k in ("total_loss", "value_loss", "reward_loss", "policy_loss", "mean_value"))
    assert first[-1]["mean_total_reward"] == first[-1]["mean_length"] == first[-1]["mean_reward_player0"]


def test_the_loops_host_twin_gives_the_same_rows(mods, first_rows):
    """device_filing=False: the games through on_games -> save_games, their outcomes from ReplayBuffer.game_outcomes."""
    assert strip(cartpole_rows(mods, False)) == strip(first_rows)


def test_the_loop_gives_the_same_rows_twice(mods, first_rows):
    assert strip(cartpole_rows(mods, True)) == strip(first_rows)


def test_the_loop_on_tictactoe_with_the_residual_network(mods):
    """The residual config cut down to 10 simulations, batch 16, 3 unroll steps; 16 envs, 2 iterations of 9 moves and 3
    steps, an evaluation of 8 games after each."""
    config = mods.loop.game_config("tictactoe", dict(num_simulations=10, batch_size=16, num_unroll_steps=3, training_steps=6))
    assert config.network == "resnet"
    loop = mods.loop.TrainingLoop("tictactoe", config, 16, 9, 3, seed=0, eval_every=1, eval_games=8)
    rows = loop.run(2)
    counted = loop.games_finished
    assert rows[-1]["training_step"] == 3 and rows[-1]["total_loss"] is not None and mods.loop.finite(rows[-1])
    assert rows[-1]["num_played_games"] == rows[-1]["games_finished"] == counted > 0
    for row in rows:
        metrics = row["eval"]
        assert metrics["opponent"] == "expert" and metrics["games"] == 8
        assert all(math.isfinite(metrics[k]) for k in ("total_reward", "episode_length", "muzero_reward", "opponent_reward"))
    loop.close()
    assert loop.replay.num_played_games == loop.games_finished >= counted
