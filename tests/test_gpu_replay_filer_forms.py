"""The six kernels behind DeviceSelfPlay.file_to (csrc/mzreplay.hip: filer_count_kernel, filer_scan_kernel,
filer_append_kernel<vec4>, filer_priorities_kernel, filer_begin_kernel, gather_priorities_kernel) and the host code around
them (mzreplay_filer_file, mzreplay_filer_sync, filer_drain), held to a one-move-at-a-time numpy model at every scan and
ring edge.  No actor, no search, no network: seeded batches (tests/replay_filer_cases.py) go through ReplayBuffer's
attach_filer / filer_begin / filer_file / sync_filing as the product calls them.

After every sync, against the model: what the sync returned, the four counters and the buffer's keys, the running
lengths, every stored game's seven arrays byte for byte, slots the round did not write unchanged, and priorities against
the oracle (tests/test_gpu_replay_edges.py assert_priorities: exact at PER_alpha = 1, rtol 2e-7 otherwise).  The cases
marked `twin` also fill a second store through save_games and compare the pair with test_gpu_replay_filer.py's
assert_same_stores: the targets of every position bit for bit and, with device sampling, twenty sampled batches.

Whether each case reaches the edge it is named for is asserted on the CPU (tests/test_replay_filer_reference.py), where
the model itself is held to the host path.  kErrList (the list of filed games had no room) is left out: the host sizes the
list for E x M games per unsynced call, so it cannot be reached without corrupting the host's own sizing."""
import importlib
import re
import types

import numpy as np
import pytest
import torch

import replay_filer_cases as rc
from test_gpu_replay_edges import (absorbing_for, all_pairs, assert_priorities, assert_targets, device_targets, oracle_batch,
                                   packed_of, plain_config)
from test_gpu_replay_filer import assert_same_stores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return types.SimpleNamespace(rb=importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
                                 sp=importlib.import_module("muzero-hypermodel_amd.self_play"),
                                 native=importlib.import_module("muzero-hypermodel_amd._native"), ro=rc.replay_oracle())


def config_of(case, alpha=0.5):
    return plain_config(case.A, case.players, case.obs_shape, case.max_moves, case.td_steps, 2, 0, rc.DISCOUNT, alpha=alpha,
                        capacity=case.capacity, batch_size=32, seed=case.seed)


def new_store(mods, case, config, device_sampling=False):
    return mods.rb.ReplayBuffer({"num_played_games": case.next_id, "num_played_steps": 0}, {}, config,
                                device_sampling=device_sampling)


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        rows = np.flatnonzero((got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)).any(axis=1))
        raise AssertionError(f"{what}: {len(rows)} of {len(got)} rows differ, first row {rows[0]}: got {got[rows[0]]!r}, "
                             f"want {want[rows[0]]!r}")


class Filed:
    """A store with a filer on the card, fed the model's batches and checked against its rounds."""

    def __init__(self, mods, case, alpha=0.5, device_sampling=False):
        self.mods, self.case, self.device_sampling = mods, case, device_sampling
        self.trace = rc.run_model(case)
        self.config = config_of(case, alpha)
        self.store = new_store(mods, case, self.config, device_sampling)
        self.twin = new_store(mods, case, self.config, device_sampling) if case.twin else None
        dev = self.store.device
        self.store.attach_filer(case.E)
        first_tp = self.trace.first_to_play
        self.first = (torch.from_numpy(self.trace.first_obs).to(dev), None if first_tp is None else torch.from_numpy(first_tp).to(dev))
        self.store.filer_begin(*self.first)
        self.keep, self.seen, self.vec4 = [], {}, set()

    def file(self, batch):
        keep = rc.upload(batch, self.store.device, self.case.misalign)
        for name in ("obs_after", "obs_next"):
            assert (keep[name].data_ptr() % 16 != 0) == (name in self.case.misalign), name
        self.vec4.add(rc.takes_vec4(self.case.obs_floats, keep["obs_after"].data_ptr(), keep["obs_next"].data_ptr()))
        self.keep.append(keep)                                 # (the filing is queued: the tensors live until the sync)
        self.store.filer_file(rc.file_moves(self.mods.native, keep, batch["actions"].shape[0], rc.S, self.case.players,
                                            batch_legal=self.case.legal_form == "batch"))

    def sync(self, rnd, where):
        case, store, ro = self.case, self.store, self.mods.ro
        if rnd.error is not None:                              # the following sync hands out the earlier calls' games
            with pytest.raises(RuntimeError, match=re.escape(rnd.error)):
                store.sync_filing()
        env, length, ids = store.sync_filing()
        self.keep.clear()
        assert [env.tolist(), length.tolist(), ids.tolist()] == [rnd.env_index, rnd.length, rnd.ids], where
        assert [store.num_played_games, len(store.buffer), store.total_samples, store.num_played_steps] == rnd.counters, where
        assert list(store.buffer) == rnd.stored_ids, where
        assert store.filer_lengths().tolist() == rnd.running, where
        games = [rnd.slots[gid % case.capacity] for gid in rnd.stored_ids]
        assert [g["id"] for g in games] == rnd.stored_ids
        if not games:
            return
        got, want = store.download_games(rnd.stored_ids), rc.padded_games(case, games)
        for key in rc.ARRAYS:
            same_bytes(getattr(got, key), want["lengths" if key == "length" else key], f"{where}: {key}")
        # slots the round did not write still hold what they held
        written = {gid for c in rnd.calls if c.refused is None for _, _, gid in c.survivors}
        now = {}
        for i, gid in enumerate(rnd.stored_ids):
            entry = store.buffer[gid]
            now[gid] = tuple(getattr(got, key)[i].tobytes() for key in rc.ARRAYS) + (
                entry["priorities"].tobytes(), np.float32(entry["game_priority"]).tobytes())
            if gid not in written:
                assert now[gid] == self.seen[gid], f"{where}: game {gid}, which the round did not write, changed"
        self.seen = now
        check = rnd.stored_ids if self.device_sampling else sorted(written & set(rnd.stored_ids))
        by_id = {gid: rc.oracle_game(ro, g) for gid, g in zip(rnd.stored_ids, games)}
        assert_priorities(store, ro, self.config, by_id, check, where)
        if self.twin is not None:
            for c in rnd.calls:
                if c.refused is None and c.n_new:
                    self.twin.save_games(packed_of(self.mods.sp, rc.padded_games(case, c.game_dicts)))
            assert_same_stores(self.twin, store, where, self.device_sampling)

    def run(self):
        for r, rnd in enumerate(self.trace.rounds):
            for batch in rnd.batches:
                self.file(batch)
            self.sync(rnd, f"{self.case.name} round {r}")
        return self

    def close(self):
        self.store.close()
        if self.twin is not None:
            self.twin.close()


def run_case(mods, case, **kwargs):
    filed = Filed(mods, case, **kwargs).run()
    filed.close()
    return filed


@pytest.mark.parametrize("case", rc.BLOCK_EDGES, ids=repr)
def test_block_edges_of_the_count_kernel(mods, case):
    run_case(mods, case)


@pytest.mark.parametrize("case", rc.SCAN_CARRY, ids=repr)
def test_scan_carry_across_chunks_of_1024_envs(mods, case):
    """filer_scan_kernel's loop over chunks: ranks of envs >= 1024 start at the total of the chunks before them."""
    run_case(mods, case)


@pytest.mark.parametrize("device_sampling", [False, True])
@pytest.mark.parametrize("case", rc.WRAP, ids=repr)
def test_more_than_1024_games_dropped_by_a_wrap_inside_a_call(mods, case, device_sampling):
    """2500 envs into 1, 5 and 1500 slots: only the last `capacity` games of the call are written, every slot once, the
    counters move as if all had been stored and evicted in turn, and the sampler adopts ids and priorities."""
    run_case(mods, case, device_sampling=device_sampling)


def test_partial_eviction_across_the_rings_end_and_the_priorities_grid_stride(mods):
    """More than 1024 stored games lose their slots (the strided LDS sum of their lengths, walking across the ring's end)
    to more than 2048 new ones (filer_priorities_kernel strides its grid)."""
    run_case(mods, rc.PARTIAL_EVICTION)


@pytest.mark.parametrize("alpha", [0.5, 1])
def test_a_game_of_260_moves_carried_across_four_calls(mods, alpha):
    """Positions >= 256 of a game: filer_priorities_kernel's inner stride, the block maximum found there."""
    run_case(mods, rc.LONG_GAME, alpha=alpha)


@pytest.mark.parametrize("case", rc.ACTION_WIDTHS, ids=repr)
def test_action_widths_with_per_move_legal_sets_and_two_players(mods, case):
    run_case(mods, case)


def test_one_legal_set_for_the_batch(mods):
    run_case(mods, rc.ONE_LEGAL_SET)


@pytest.mark.parametrize("case", rc.OBS_COPIES, ids=repr)
def test_observation_copies_take_the_path_the_pointers_allow(mods, case):
    """filer_append_kernel<true> needs obs_floats % 4 == 0 and both rings 16-byte aligned; anything else the scalar copy."""
    filed = run_case(mods, case)
    assert filed.vec4 == {case.obs_floats % 4 == 0 and not case.misalign}


def test_calls_between_two_syncs(mods):
    """Three calls, one sync: the list's drain inside mzreplay_filer_file, the list growing, Call::list_base.  The result
    equals three synced calls on a second store."""
    case = rc.BETWEEN_SYNCS
    one = Filed(mods, case).run()
    each = Filed(mods, case)
    synced = []
    for batch in each.trace.rounds[0].batches:
        each.file(batch)
        synced.append(each.store.sync_filing())
    rnd = each.trace.rounds[0]
    for i, want in enumerate((rnd.env_index, rnd.length, rnd.ids)):
        assert np.concatenate([s[i] for s in synced]).tolist() == want
    assert_same_stores(each.store, one.store, case.name, False)
    one.close()
    each.close()


def test_a_reanalysed_slot_is_overwritten_and_forgotten(mods):
    """Capacity 4, every stored game reanalysed, then a call that overwrites two of the four: the new games' targets
    bootstrap from their own root values, the other two still from Reanalyse's."""
    case, ro = rc.REANALYSED, mods.ro
    filed = Filed(mods, case)
    first, second = filed.trace.rounds
    filed.file(first.batches[0])
    filed.sync(first, "reanalysed round 0")
    rs = np.random.RandomState(7)
    fresh = {gid: (rs.standard_normal(3) * 3).astype(np.float32) for gid in first.stored_ids}
    for gid, values in fresh.items():
        filed.store.set_reanalysed_values(gid, values)
    filed.file(second.batches[0])
    filed.sync(second, "reanalysed round 1")
    games = {}
    for gid in second.stored_ids:
        g = second.slots[gid % case.capacity]
        games[gid] = ro.Game(g["observations"], g["actions"], g["rewards"], g["to_play"], g["child_visits"], g["root_values"])
        if gid in fresh:
            games[gid].reanalysed = fresh[gid]
    assert sorted(gid for gid in games if games[gid].reanalysed is not None) == [2, 3]
    lengths = {gid: 3 for gid in games}
    pairs = all_pairs(second.stored_ids, lengths)
    absorbing = absorbing_for(rs, pairs, lengths, filed.config.num_unroll_steps + 1, case.A)
    got = device_targets(filed.store, pairs, absorbing, sizes=(5, 64))
    assert_targets(got, oracle_batch(ro, filed.config, games, pairs, absorbing), case.name)
    for gid in (2, 3):                                          # and it matters: without Reanalyse's values they differ
        games[gid].reanalysed = None
    assert not np.array_equal(got["value"], oracle_batch(ro, filed.config, games, pairs, absorbing)["value"])
    filed.close()


def test_a_game_that_outgrows_max_moves_refuses_the_call(mods):
    """kErrOverflow on the device: the sync raises, store, counters and running lengths are unchanged, the next call works."""
    run_case(mods, rc.OVERFLOW)


def test_a_refused_call_between_unsynced_calls(mods):
    """Calls good, bad (a legal action of A), good with no sync between: the third is refused with the second, the sync
    raises mzhist_file's message, the following sync hands out the first call's games, and the store equals the model that
    filed only those.  (The list's drain inside the third call used to erase the error word: the sync then reported
    nothing and the third call was filed.)"""
    run_case(mods, rc.REFUSED)
