"""Finished self-play games filed into the replay store on the device (DeviceSelfPlay.file_to; include/mzreplay.h
mzreplay_filer_*, csrc/replay_filer.h) against the host path it replaces, in twin runs: the same weights and seeds, actor A
through on_games -> ReplayBuffer.save_games into store A, actor B with file_to(store B), the same sequence of play_moves
sizes and a final flush().  The two stores must then be equal bit for bit: counters, buffer keys and lengths, every stored
game read back in all seven arrays, priorities, the targets of every (game, position) pair and -- with device sampling --
twenty sampled batches.  The filer's index arithmetic alone is held to the host path on the CPU
(tests/test_replay_filer_cpu.py)."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import synthetic_model
from replay_filer_cases import file_moves

pytestmark = pytest.mark.gpu
START = {"num_played_games": 0, "num_played_steps": 0}
ARRAYS = ("length", "observations", "actions", "rewards", "to_play", "child_visits", "root_values")


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return (importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
            importlib.import_module("muzero-hypermodel_amd.self_play"),
            importlib.import_module("muzero-hypermodel_amd.models"))


def games(name):
    return importlib.import_module(f"muzero-hypermodel_amd.games.{name}")


def assert_same_stores(a, b, what, device_sampling):
    assert (a.num_played_games, a.num_played_steps, a.total_samples) == (b.num_played_games, b.num_played_steps, b.total_samples), what
    assert list(a.buffer) == list(b.buffer), what
    ids = list(a.buffer)
    assert [a.buffer[g]["length"] for g in ids] == [b.buffer[g]["length"] for g in ids], what
    assert all(b.buffer[g]["history"] is None for g in ids)
    if not ids:
        return 0
    ga, gb = a.download_games(ids), b.download_games(ids)
    for key in ARRAYS:
        assert getattr(ga, key).tobytes() == getattr(gb, key).tobytes(), f"{what}: {key}"
    assert ga.length.tolist() == [a.buffer[g]["length"] for g in ids]
    if a.config.PER:
        for g in ids:
            assert a.buffer[g]["priorities"].tobytes() == b.buffer[g]["priorities"].tobytes(), f"{what}: priorities of game {g}"
            assert np.float32(a.buffer[g]["game_priority"]).tobytes() == np.float32(b.buffer[g]["game_priority"]).tobytes(), what
    # the targets of every stored position (absorbing actions 0: nothing is drawn here)
    pairs = [(g, p) for g in ids for p in range(a.buffer[g]["length"])]
    slots = np.array([g % a.capacity for g, _ in pairs], np.int32)
    positions = np.array([p for _, p in pairs], np.int32)
    absorbing = np.zeros((len(pairs), a.U1), np.int32)
    ta, tb = a.make_targets(slots, positions, absorbing), b.make_targets(slots, positions, absorbing)
    for key in ta:
        assert ta[key].cpu().numpy().tobytes() == tb[key].cpu().numpy().tobytes(), f"{what}: target {key}"
    if device_sampling:
        for draw in range(20):
            ia, ba = a.get_batch()
            ib, bb = b.get_batch()
            assert ia.tolist() == ib.tolist(), f"{what}: batch {draw} indices"
            for x, y in zip(ba, bb):
                assert (x is None) == (y is None)
                if x is not None:
                    assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"{what}: batch {draw}"
    return len(pairs)


def twin_run(mods, game, config, weights, E, sizes, temperature=1.0, threshold=None, device_sampling=False, seed=0,
             use_graph=True, between=None, want_short=False, want_two_games=False, want_overflow=False):
    """Plays the same batches through both paths; returns (store A, store B, actor A, actor B, filed batches of B)."""
    rb_mod, sp, _ = mods
    store_a = rb_mod.ReplayBuffer(START, {}, config, device_sampling=device_sampling)
    store_b = rb_mod.ReplayBuffer(START, {}, config, device_sampling=device_sampling)
    actor_a = sp.DeviceSelfPlay({"weights": weights}, game, config, seed, E, use_graph=use_graph)
    actor_b = sp.DeviceSelfPlay({"weights": weights}, game, config, seed, E, use_graph=use_graph)
    actor_b.file_to(store_b)
    filed, host_batches = [], []

    def host_games(batch):
        host_batches.append((batch.env_index.copy(), batch.length.copy()))
        store_a.save_games(batch)
    short = False
    for i, n in enumerate(sizes):
        played_a = actor_a.play_moves(n, temperature, on_games=host_games, temperature_threshold=threshold)
        played_b = actor_b.play_moves(n, temperature, on_games=filed.append, temperature_threshold=threshold)
        if i % 2 == 0 or between is not None:
            # both forms: a batch's games leave in flush(), or inside the next play_moves while the GPU runs that batch
            actor_a.flush(on_games=host_games)
            actor_b.flush(on_games=filed.append)
        assert np.array_equal(played_a, played_b), f"batch {i}: the twins played different moves"
        short |= bool((played_b < n).any())
        if between is not None:
            between(i, store_a, store_b)
    actor_a.flush(on_games=host_games)
    actor_b.flush(on_games=filed.append)
    assert actor_a.moves_played == actor_b.moves_played and actor_a.games_finished == actor_b.games_finished > 0
    assert actor_b.searched_moves == actor_b.moves_played
    # what on_games received: the same games in the same order, with the ids the store gave them
    assert len(filed) == len(host_batches)
    for f, (env, length) in zip(filed, host_batches):
        assert isinstance(f, sp.FiledGames)
        assert np.array_equal(f.env_index, env) and np.array_equal(f.length, length)
    ids = np.concatenate([f.game_id for f in filed])
    if between is None:
        assert np.array_equal(ids, np.arange(len(ids)))
    assert np.array_equal(actor_b._len, actor_a._len)
    if want_short:
        assert short, "no env came back with fewer moves than the batch: the unplayed-suffix rule was not exercised"
    if want_two_games:
        assert any(len(f.env_index) != len(set(f.env_index.tolist())) for f in filed), "no env finished two games in one call"
    if want_overflow:
        assert any(len(f) > store_b.capacity for f in filed), "no call finished more games than the store has slots"
    return store_a, store_b, actor_a, actor_b, filed


def close_all(*things):
    for t in things:
        t.close()


def cartpole_weights(pkg, ties):
    from test_gpu_moves import cartpole_setup
    config, model = cartpole_setup(pkg, ties)
    return config, {k: v.cpu() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("device_sampling", [False, True])
def test_cartpole_predrawn_batches_with_stalls(mods, pkg, device_sampling):
    """The fused pre-drawn form at T = 1 with weights whose searches tie at unpredictable moves: envs stall mid-batch and
    come back with fewer moves than the batch; games end at a short move limit, so the capacity-4 ring wraps across
    calls."""
    config, weights = cartpole_weights(pkg, "some")
    config.max_moves, config.td_steps, config.replay_buffer_size, config.batch_size = 9, 3, 4, 32
    a, b, aa, ab, _ = twin_run(mods, "cartpole", config, weights, 24, (5, 7, 4, 6, 8, 6, 7), device_sampling=device_sampling,
                               want_short=True)
    assert b.num_played_games > 2 * b.capacity        # the ring wrapped across the calls
    assert assert_same_stores(a, b, "cartpole stalls", device_sampling) > 20
    close_all(aa, ab, a, b)


def test_cartpole_more_games_in_a_call_than_slots(mods, pkg):
    """Capacity 5 with 64 envs: one call finishes more games than the store has slots; only the last five are written and
    the counters move as if all had been stored and evicted in turn."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 6, 2, 5
    a, b, aa, ab, _ = twin_run(mods, "cartpole", config, weights, 64, (8, 5, 9), want_overflow=True)
    assert len(b.buffer) == 5
    assert_same_stores(a, b, "capacity 5", False)
    close_all(aa, ab, a, b)


def test_cartpole_temperature_threshold(mods, pkg):
    """A temperature threshold takes the device-input form of the batch, and the rule needs the running games' lengths:
    they come from the device filer."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 11, 3, 40
    a, b, aa, ab, _ = twin_run(mods, "cartpole", config, weights, 16, (6, 7, 5, 9), threshold=4)
    assert_same_stores(a, b, "cartpole threshold", False)
    close_all(aa, ab, a, b)


def tictactoe_fc(models_mod):
    config = games("tictactoe").MuZeroConfig()
    config.network, config.encoding_size = "fullyconnected", 8
    config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
    config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
    config.num_simulations = 20
    config.temperature_threshold = None
    torch.manual_seed(0)
    return config, models_mod.MuZeroNetwork(config).get_weights()


@pytest.mark.parametrize("device_sampling", [False, True])
def test_tictactoe_two_players_two_games_per_call(mods, device_sampling):
    """Two players, legal sets that change every move, and max_moves = 3 with 8-move batches: every env finishes at least
    two games in one call, so a finished game's successor takes the NEXT move's player to move."""
    config, weights = tictactoe_fc(mods[2])
    config.max_moves, config.td_steps, config.replay_buffer_size, config.batch_size = 3, 2, 300, 64
    a, b, aa, ab, _ = twin_run(mods, "tictactoe", config, weights, 48, (8, 8, 5), device_sampling=device_sampling,
                               want_two_games=True)
    assert_same_stores(a, b, "tictactoe max_moves 3", device_sampling)
    close_all(aa, ab, a, b)


def test_tictactoe_whole_games_and_host_games_in_between(mods):
    """Whole games (5-9 plies), and games added with save_game between two filings: they land where the host path puts
    them, ids and slots shared by both producers."""
    rb_mod, sp, models_mod = mods
    config, weights = tictactoe_fc(models_mod)
    config.td_steps, config.replay_buffer_size = 4, 70
    extra = []

    def between(i, store_a, store_b):
        if i == 0:
            ids = list(store_a.buffer)[:3]
            extra.extend(store_a.download_games(ids).history(k) for k in range(3))
        if i in (0, 1):
            for gh in extra:
                for store in (store_a, store_b):
                    fresh = sp.GameHistory()
                    for key in ("observation_history", "action_history", "reward_history", "to_play_history",
                                "child_visits", "root_values"):
                        setattr(fresh, key, list(getattr(gh, key)))
                    store.save_game(fresh)
    a, b, aa, ab, filed = twin_run(mods, "tictactoe", config, weights, 32, (9, 6, 11), between=between)
    ids = np.concatenate([f.game_id for f in filed])
    assert len(np.unique(ids)) == len(ids) and b.num_played_games == len(ids) + 6
    assert sum(1 for e in b.buffer.values() if e["history"] is not None) > 0
    a_hist, b_hist = a.get_buffer(), b.get_buffer()
    assert list(a_hist) == list(b_hist)
    for g in a_hist:
        if b.buffer[g]["history"] is None:               # filed on the device: read back, a GameHistory like the host's
            assert b_hist[g].action_history == a.download_games([g]).history(0).action_history
    # (entries the host added carry histories on both sides; compare what the stores hold)
    for store in (a, b):
        for e in store.buffer.values():
            e["history"] = None
    assert_same_stores(a, b, "tictactoe with host games in between", False)
    close_all(aa, ab, a, b)


def test_connect4_lockstep_residual_network(mods):
    """The lock-step form: a small residual network searched with the captured simulation loop, inputs recorded per move
    in the engine's device ring."""
    config = games("connect4").MuZeroConfig()
    config.blocks, config.channels, config.num_simulations = 1, 16, 10
    config.max_moves, config.td_steps, config.replay_buffer_size = 12, 3, 60
    config.temperature_threshold = None
    _, weights = synthetic_model(mods[2], config, "cpu")
    a, b, aa, ab, _ = twin_run(mods, "connect4", config, weights, 24, (9, 11, 6))
    assert_same_stores(a, b, "connect4 lock-step", False)
    close_all(aa, ab, a, b)


def test_gomoku_121_actions(mods):
    config = games("gomoku").MuZeroConfig()
    config.blocks, config.channels, config.num_simulations = 1, 8, 6
    config.max_moves, config.td_steps, config.replay_buffer_size = 10, 3, 20
    config.temperature_threshold = None
    _, weights = synthetic_model(mods[2], config, "cpu")
    a, b, aa, ab, _ = twin_run(mods, "gomoku", config, weights, 16, (7, 9, 8), seed=30)
    assert b.num_played_games > b.capacity
    assert_same_stores(a, b, "gomoku", False)
    close_all(aa, ab, a, b)


def test_reanalysed_slot_is_overwritten_and_forgotten(mods, pkg):
    """A slot that set_reanalysed_values touched is overwritten by a later filing: the new game's targets bootstrap from
    its own root values again (has_reanalysed back to 0), as after mzreplay_add_games."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 8, 2, 6
    touched = []

    def between(i, store_a, store_b):
        if i == 0:
            for gid in list(store_b.buffer):
                n = store_b.buffer[gid]["length"]
                values = np.linspace(5.0, 9.0, n).astype(np.float32)
                store_a.set_reanalysed_values(gid, values)
                store_b.set_reanalysed_values(gid, values)
                touched.append(gid % store_b.capacity)
    a, b, aa, ab, _ = twin_run(mods, "cartpole", config, weights, 12, (9, 9, 9), between=between)
    assert touched and b.num_played_games >= 3 * b.capacity   # every touched slot was overwritten since
    assert_same_stores(a, b, "reanalysed slots", False)
    close_all(aa, ab, a, b)


def test_bad_legal_sets_are_refused_without_touching_the_store(mods):
    """Argument checking: a legal action of A, then a legal count of A + 1, in an otherwise valid batch.  The sync
    returns mzhist_file's message, the store is unchanged, and later calls work."""
    rb_mod, sp, _ = mods
    native = importlib.import_module("muzero-hypermodel_amd._native")
    config = games("tictactoe").MuZeroConfig()
    config.max_moves, config.replay_buffer_size = 4, 8
    store = rb_mod.ReplayBuffer(START, {}, config)
    E, M, A = 5, 2, 9
    dev = store.device
    obs_shape = tuple(int(v) for v in config.observation_shape)
    store.attach_filer(E)
    store.filer_begin(torch.zeros((E,) + obs_shape, device=dev), torch.zeros(E, dtype=torch.int32, device=dev))
    keep = dict(actions=torch.zeros((M, E), dtype=torch.int32, device=dev),
                visits=torch.ones((M, E, A), dtype=torch.int32, device=dev),
                rvs=torch.zeros((M, E), dtype=torch.float64, device=dev),
                legal=torch.arange(A, dtype=torch.int32, device=dev).repeat(M, E, 1).contiguous(),
                num_legal=torch.full((M, E), A, dtype=torch.int32, device=dev),
                to_play=torch.zeros((M, E), dtype=torch.int32, device=dev),
                last=torch.zeros(E, dtype=torch.int32, device=dev),
                rewards=torch.ones((M, E), dtype=torch.float32, device=dev),
                done=torch.tensor([[0] * E, [1] * E], dtype=torch.uint8, device=dev),
                obs_after=torch.ones((M, E) + obs_shape, device=dev), obs_next=torch.zeros((M, E) + obs_shape, device=dev))

    def moves():
        return file_moves(native, keep, M, 10, 2)
    store.filer_file(moves())
    env, length, ids = store.sync_filing()
    assert env.tolist() == list(range(E)) and length.tolist() == [2] * E and ids.tolist() == list(range(E))
    before = (store.num_played_games, store.num_played_steps, store.total_samples, list(store.buffer))
    stored = store.download_games(list(store.buffer))
    for corrupt in ("action", "count"):
        if corrupt == "action":
            keep["legal"][1, 3, 4] = A
        else:
            keep["num_legal"][0, 2] = A + 1
        store.filer_file(moves())
        with pytest.raises(RuntimeError, match="mzhist_file: a legal-action count outside"):
            store.sync_filing()
        keep["legal"][1, 3, 4] = 4
        keep["num_legal"][0, 2] = A
        assert (store.num_played_games, store.num_played_steps, store.total_samples, list(store.buffer)) == before
        again = store.download_games(list(store.buffer))
        for key in ARRAYS:
            assert getattr(stored, key).tobytes() == getattr(again, key).tobytes(), key
        assert store.filer_lengths().tolist() == [0] * E
    store.filer_file(moves())                              # and a later call works
    env, length, ids = store.sync_filing()
    assert ids.tolist() == list(range(E, 2 * E)) and store.num_played_games == 2 * E and len(store.buffer) == 8
    store.close()


def test_what_file_to_refuses(mods, pkg):
    rb_mod, sp, _ = mods
    config, weights = cartpole_weights(pkg, False)
    config.max_moves = 6
    store = rb_mod.ReplayBuffer(START, {}, config)
    actor = sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 0, 8)
    actor.file_to(store)
    with pytest.raises(ValueError):
        actor.file_to(store)
    other = sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 0, 8)
    with pytest.raises(NotImplementedError, match="file_to"):
        other.file_to(store)                               # one actor files into one store
    other.play_moves(2, 1.0)
    other.flush()
    with pytest.raises(ValueError, match="before the first move"):
        other.file_to(rb_mod.ReplayBuffer(START, {}, config))
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.step(1.0)
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.play_moves(2, 1.0, on_game=lambda e, gh: None)
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.play_moves(2, 1.0, opponent="random")
    actor.play_moves(7, 1.0)
    actor.flush()
    assert store.num_played_games == actor.games_finished >= 8
    close_all(actor, other, store)
