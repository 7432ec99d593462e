"""Several actors filing into one replay store on the device (include/mzreplay.h: the store numbers games in the order of
the mzreplay_filer_file calls made on it, whatever stream each call runs on).

* Synthetic rings (tests/replay_filer_cases.py make_batch) filed through K filers on K streams, interleaved as the
  scenarios of tests/replay_filer_shared_cases.py say, against the numpy model of K filers over one store: what every
  filer's sync hands out, the four counters, the buffer's keys, the running lengths, every stored game's seven arrays byte
  for byte and the priorities (PER_alpha = 1: exact).  In the order scenarios the stream of the filer that files FIRST is
  held up by a sleep kernel of a few milliseconds ahead of each of its calls: without the store's "last filing" event the
  other filer's kernels would run first and take its ids.  The sleep only delays a stream.
* PipelinedDeviceSelfPlay.file_to against a twin run through on_games -> save_games (tests/test_gpu_replay_filer.py
  assert_same_stores), with and without prefetch, with the device sampler, and two DeviceSelfPlay actors into one buffer.

Whether each scenario reaches the edge it is named for is asserted on the CPU (tests/test_replay_filer_shared_cpu.py)."""
import ctypes
import importlib
import re
import types

import numpy as np
import pytest
import torch

import replay_filer_cases as rc
import replay_filer_shared_cases as sc
from test_gpu_replay_edges import assert_priorities, plain_config
from test_gpu_replay_filer import START, assert_same_stores, cartpole_weights, close_all, tictactoe_fc
from test_gpu_replay_filer_forms import same_bytes

pytestmark = pytest.mark.gpu
SLEEP_CYCLES = 10_000_000     # torch.cuda._sleep: a few milliseconds, far longer than the other filer's four launches


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return types.SimpleNamespace(rb=importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
                                 sp=importlib.import_module("muzero-hypermodel_amd.self_play"),
                                 models=importlib.import_module("muzero-hypermodel_amd.models"),
                                 native=importlib.import_module("muzero-hypermodel_amd._native"), ro=rc.replay_oracle())


# ---- K filers, K streams, synthetic rings -----------------------------------------------------------------------------
def run_scenario(mods, scn, delay=None):
    """Files the scenario's batches, each through its filer on its filer's stream, syncs, and holds everything the store
    and the filers show to the model's trace.  delay = k: a sleep kernel ahead of each of filer k's calls on its stream."""
    trace = sc.run_model(scn)
    config = plain_config(scn.A, scn.players, scn.obs_shape, scn.max_moves, scn.td_steps, 2, 0, rc.DISCOUNT, alpha=1,
                          capacity=scn.capacity, batch_size=32, seed=scn.seed)
    store = mods.rb.ReplayBuffer({"num_played_games": scn.next_id, "num_played_steps": 0}, {}, config)
    dev = store.device
    streams = [torch.cuda.Stream(device=dev) for _ in scn.envs]
    filers = [store.attach_filer(E) for E in scn.envs]
    assert len({f.handle.value for f in filers}) == len(scn.envs)
    firsts = [(torch.from_numpy(obs).to(dev), None if tp is None else torch.from_numpy(tp).to(dev)) for obs, tp in trace.first]
    uploads = [rc.upload(step.batch, dev) for step in trace.steps]         # (alive until the sync)
    torch.cuda.synchronize(dev)
    for k, filer in enumerate(filers):
        with torch.cuda.stream(streams[k]):
            filer.begin(*firsts[k])
    for step, keep in zip(trace.steps, uploads):
        with torch.cuda.stream(streams[step.k]):
            if delay == step.k:
                torch.cuda._sleep(SLEEP_CYCLES)
            filers[step.k].file(rc.file_moves(mods.native, keep, step.batch["actions"].shape[0], rc.S, scn.players,
                                              batch_legal=scn.legal_form == "batch"))
    assert store.filing_pending
    errors = [error for error, _ in trace.syncs if error is not None]
    if errors:                                             # the failing sync keeps everything; the next one books it
        with pytest.raises(RuntimeError, match=re.escape(errors[0])):
            store.sync_filing()
        assert len(store.buffer) == 0
    assert store.sync_filing() is None                     # (several filers: each takes its own list)
    for k, filer in enumerate(filers):
        env, length, ids = filer.take_filed()
        want = trace.syncs[k][1]
        assert [env.tolist(), length.tolist(), ids.tolist()] == [[g[i] for g in want] for i in range(3)], f"{scn.name}: filer {k}"
        assert (env.dtype, length.dtype, ids.dtype) == (np.int32, np.int32, np.int64)
    assert [store.num_played_games, len(store.buffer), store.total_samples, store.num_played_steps] == trace.counters
    assert list(store.buffer) == trace.stored_ids
    for k, filer in enumerate(filers):
        assert filer.lengths().tolist() == trace.running[k], f"{scn.name}: running lengths of filer {k}"
    games = [trace.slots[gid % scn.capacity] for gid in trace.stored_ids]
    assert [g["id"] for g in games] == trace.stored_ids
    got, want = store.download_games(trace.stored_ids), rc.padded_games(scn, games)
    for key in rc.ARRAYS:
        same_bytes(getattr(got, key), want["lengths" if key == "length" else key], f"{scn.name}: {key}")
    by_id = {gid: rc.oracle_game(mods.ro, g) for gid, g in zip(trace.stored_ids, games)}
    assert_priorities(store, mods.ro, config, by_id, trace.stored_ids, scn.name)
    return store, filers


@pytest.mark.parametrize("scn, delayed", [(sc.ORDER_AB, sc.A), (sc.ORDER_BA, sc.B)], ids=["A_first", "B_first"])
def test_ids_follow_the_host_call_order_against_the_streams(mods, scn, delayed):
    """E = 3 and E = 5, M = 4, a 4-slot store, calls A, B, A, B (and B, A, B, A) on two streams; the stream of the filer
    that calls first sleeps ahead of each of its calls."""
    store, _ = run_scenario(mods, scn, delay=delayed)
    store.close()


def test_three_filers_two_players_a_ring_that_wraps(mods):
    store, _ = run_scenario(mods, sc.THREE)
    store.close()


def test_scan_carry_on_a_non_zero_shared_base(mods):
    """The second filer's 1030 envs are ranked from the id the first filer's call left in the shared block."""
    store, _ = run_scenario(mods, sc.SCAN_BASE, delay=sc.A)
    store.close()


def test_a_refusal_stays_with_its_filer(mods):
    """A's second call has a legal action of A: B's calls before and after it file with contiguous ids, A's failing sync
    keeps A's first call's games, and the store equals the model."""
    store, _ = run_scenario(mods, sc.REFUSAL)
    store.close()


def test_the_one_filer_sync_names_the_new_entry_on_a_store_with_two_filers(mods):
    scn = sc.ORDER_AB
    config = plain_config(scn.A, scn.players, scn.obs_shape, scn.max_moves, scn.td_steps, 2, 0, rc.DISCOUNT, capacity=4)
    store = mods.rb.ReplayBuffer(START, {}, config)
    lib = mods.native.load()
    one = store.attach_filer(3)
    n, first = ctypes.c_int32(), ctypes.c_int64()
    assert lib.mzreplay_filer_sync(one.handle, ctypes.byref(n), None, None, ctypes.byref(first), None, None) == 0
    assert (n.value, first.value) == (0, 0)                # one filer: as before
    store.attach_filer(5)
    assert lib.mzreplay_filer_sync(one.handle, ctypes.byref(n), None, None, ctypes.byref(first), None, None) != 0
    assert b"mzreplay_filer_sync_ids" in lib.mzreplay_last_error(store._h)
    with pytest.raises(RuntimeError, match="name the filer"):
        store.filer_lengths()                              # the argument-free forms need exactly one filer
    store.close()


# ---- the actors -------------------------------------------------------------------------------------------------------
def pipelined_twins(mods, game, config, weights, E, sizes, prefetch, device_sampling=False):
    """The same batches through on_games -> save_games (store A) and through file_to (store B), two groups each."""
    store_a = mods.rb.ReplayBuffer(START, {}, config, device_sampling=device_sampling)
    store_b = mods.rb.ReplayBuffer(START, {}, config, device_sampling=device_sampling)
    actor_a = mods.sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 0, E, groups=2)
    actor_b = mods.sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 0, E, groups=2)
    actor_b.file_to(store_b)
    host, filed = [], []

    def host_games(batch):
        host.append((batch.env_index.copy(), batch.length.copy()))
        store_a.save_games(batch)
    for i, n in enumerate(sizes):
        ahead = prefetch and i + 1 < len(sizes)            # (the last call leaves nothing queued behind it)
        played_a = actor_a.play_moves(n, 1.0, on_games=host_games, temperature_threshold=0, prefetch=ahead)
        played_b = actor_b.play_moves(n, 1.0, on_games=filed.append, temperature_threshold=0, prefetch=ahead)
        assert np.array_equal(played_a, played_b), f"batch {i}: the twins played different moves"
    actor_a.flush(on_games=host_games)
    actor_b.flush(on_games=filed.append)
    assert actor_a.moves_played == actor_b.moves_played and actor_a.games_finished == actor_b.games_finished > 0
    # what on_games received: the same games in the same order (per batch: group 0, then group 1), global env indices,
    # and ids in the order they were handed out
    assert len(filed) == len(host)
    for f, (env, length) in zip(filed, host):
        assert isinstance(f, mods.sp.FiledGames)
        assert np.array_equal(f.env_index, env) and np.array_equal(f.length, length)
    assert {int(e) >= E // 2 for f in filed for e in f.env_index} == {False, True}
    ids = np.concatenate([f.game_id for f in filed])
    assert np.array_equal(ids, np.arange(len(ids)))
    return store_a, store_b, actor_a, actor_b


def tictactoe_16(mods):
    config, weights = tictactoe_fc(mods.models)
    config.td_steps, config.replay_buffer_size, config.batch_size = 4, 40, 32
    return config, weights


@pytest.mark.parametrize("prefetch", [False, True])
def test_pipelined_tictactoe_twin_stores(mods, prefetch):
    """TicTacToe FC-16, 16 envs in two groups, 3 batches of 5 moves."""
    config, weights = tictactoe_16(mods)
    a, b, aa, ab = pipelined_twins(mods, "tictactoe", config, weights, 16, (5, 5, 5), prefetch)
    assert assert_same_stores(a, b, f"pipelined tictactoe prefetch={prefetch}", False) > 0
    close_all(aa, ab, a, b)


@pytest.mark.parametrize("prefetch", [False, True])
def test_pipelined_cartpole_twin_stores_that_wrap(mods, pkg, prefetch):
    """CartPole, 8 envs in two groups, 3 batches of 12 moves into 6 slots: a group's call evicts the other group's games."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 9, 3, 6
    a, b, aa, ab = pipelined_twins(mods, "cartpole", config, weights, 8, (12, 12, 12), prefetch)
    assert b.num_played_games > 2 * b.capacity and len(b.buffer) == 6
    assert_same_stores(a, b, f"pipelined cartpole prefetch={prefetch}", False)
    close_all(aa, ab, a, b)


def test_the_sampler_adopts_every_groups_games(mods):
    """device_sampling=True fed by the pipelined actor: the index batches, weights and targets of twenty get_batch() calls
    equal the host-filed twin's."""
    config, weights = tictactoe_16(mods)
    a, b, aa, ab = pipelined_twins(mods, "tictactoe", config, weights, 16, (5, 5, 5), False, device_sampling=True)
    assert_same_stores(a, b, "pipelined tictactoe, device sampling", True)
    close_all(aa, ab, a, b)


def test_what_the_pipelined_actor_refuses_after_file_to(mods):
    config, weights = tictactoe_16(mods)
    store = mods.rb.ReplayBuffer(START, {}, config)
    actor = mods.sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 8, groups=2)
    actor.file_to(store)
    with pytest.raises(ValueError):
        actor.file_to(store)
    other = mods.sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 8, groups=2)
    with pytest.raises(NotImplementedError, match="shared=True"):
        other.file_to(store)                               # (nothing was attached: the store still has two filers)
    assert len(store.filers) == 2
    other.close()
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.step(1.0)
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.play_moves(2, 1.0, on_game=lambda e, gh: None, temperature_threshold=0)
    with pytest.raises(NotImplementedError, match="file_to"):
        actor.play_moves(2, 1.0, temperature_threshold=0, opponent="random")
    close_all(actor, store)


def test_two_actors_file_into_one_buffer_in_call_order(mods, pkg):
    """Two DeviceSelfPlay actors (8 and 6 envs, seeds of their own) file_to one buffer (the second with shared=True), their
    play_moves alternating; host
    twins hand the same games to a second buffer through save_games in the same call order.  Ids, counters and keys are
    also held to ReplayBuffer._add's bookkeeping in numpy, fed the lengths in call order."""
    config, weights = cartpole_weights(pkg, False)
    config.max_moves, config.td_steps, config.replay_buffer_size = 9, 3, 10
    store_a, store_b = mods.rb.ReplayBuffer(START, {}, config), mods.rb.ReplayBuffer(START, {}, config)
    shapes = ((0, 8), (100, 6))
    hosts = [mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, seed, E) for seed, E in shapes]
    filing = [mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, seed, E) for seed, E in shapes]
    filing[0].file_to(store_b)
    with pytest.raises(NotImplementedError, match="shared=True"):
        filing[1].file_to(store_b)                         # joining a store that has an actor is asked for, never a default
    filing[1].file_to(store_b, shared=True)
    model = sc.HostOrder(store_b.capacity)
    want_ids, got = [[], []], [[], []]

    def host_games(k):
        def on_games(batch):
            ids, _ = model.add([dict(length=int(n)) for n in batch.length])
            want_ids[k].append((batch.env_index.tolist(), batch.length.tolist(), ids))
            store_a.save_games(batch)
        return on_games

    def filed_games(k):
        return lambda f: got[k].append((f.env_index.tolist(), f.length.tolist(), f.game_id.tolist()))
    for n in (7, 5, 9):
        for k in (0, 1):
            hosts[k].play_moves(n, 1.0, on_games=host_games(k))
            filing[k].play_moves(n, 1.0, on_games=filed_games(k))
    for k in (1, 0):                                       # (the order of the flushes is a call order like any other)
        hosts[k].flush(on_games=host_games(k))
        filing[k].flush(on_games=filed_games(k))
    assert got == want_ids and all(want_ids)
    assert any(np.any(np.diff(sum((g[2] for g in got[k]), [])) > 1) for k in (0, 1)), "the actors' ids never interleaved"
    assert [store_b.num_played_games, len(store_b.buffer), store_b.total_samples, store_b.num_played_steps] == model.counters()
    assert list(store_b.buffer) == sorted(model.lengths_of) and store_b.num_played_games > store_b.capacity
    assert_same_stores(store_a, store_b, "two actors, one buffer", False)
    close_all(*hosts, *filing, store_a, store_b)
