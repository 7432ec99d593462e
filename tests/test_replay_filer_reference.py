"""The model the device filer is held to (tests/replay_filer_cases.py FilerModel) against the host path it restates,
whether every named case reaches the condition it exists for, and whether the model can tell the filer's rules apart at
all.  Host code only: the card's side is tests/test_gpu_replay_filer_forms.py.

* the model == the native HistoryFiler (mzhist_*: running lengths and every finished game, field by field) and ==
  HostStore, ReplayBuffer._add's bookkeeping (ids, slots, which games stay, all four counters), on the small cases;
  the oracle's initial priorities are defined over every game the model stores;
* `reaches()` of every case, on the model alone: conditions, not measurements;
* four mutations of the model -- first-fit ids, `dropped` off by one, 1 - to_play as a new game's first player, the carry
  dropped at a chunk edge -- each change what it says about the cases named for them."""
import importlib

import numpy as np
import pytest

import replay_filer_cases as rc
from test_replay_filer_cpu import HostStore

SMALL = [c for c in rc.CASES if c.small]


def host_arguments(batch, players):
    """A make_batch dict as HistoryFiler.file takes it: moves_done for the prefix rule, the players as [M, E] arrays."""
    actions = batch["actions"]
    M, E = actions.shape
    moves_done = np.array([next((m for m in range(M) if actions[m, e] < 0), M) for e in range(E)], np.int32)
    out = dict(moves_done=moves_done, actions=np.maximum(actions, 0), visits=batch["visits"],
               root_value_sum=batch["root_value_sum"])
    extra = {}
    if players > 1:
        extra["to_play_after"] = (1 - batch["to_play"]).astype(np.int32)
        extra["to_play_next"] = np.concatenate([batch["to_play"][1:], batch["to_play_last"][None]]).astype(np.int32)
    return out, extra


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_the_model_equals_the_host_path(pkg, case):
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    ro = rc.replay_oracle()
    trace = rc.run_model(case)
    filer = sp.HistoryFiler(case.E, case.max_moves, case.obs_shape, case.A)
    filer.begin(trace.first_obs, trace.first_to_play)
    store = HostStore(case.capacity, next_id=case.next_id)
    for rnd in trace.rounds:
        synced = []
        for batch, call in zip(rnd.batches, rnd.calls):
            out, extra = host_arguments(batch, case.players)
            args = (out, batch["legal"], batch["num_legal"], rc.S, batch["rewards"], batch["done"], batch["obs_after"],
                    batch["obs_next"])
            assert call.played == out["moves_done"].tolist()
            if call.refused is not None:
                if call is next(c for c in rnd.calls if c.refused is not None):    # the call that raised it
                    with pytest.raises(RuntimeError, match=call.refused[:30]):
                        filer.file(*args, **extra)
                continue                                   # (a refused call files nothing, on either side)
            got = filer.file(*args, **extra)
            env = [] if got is None else got.env_index.tolist()
            assert env == [g[0] for g in call.games]
            assert ([] if got is None else got.length.tolist()) == [g[1] for g in call.games]
            ids = store.add([g[1] for g in call.games])
            assert ids == [g[2] for g in call.games]
            assert call.n_new == len(ids) and call.dropped == max(0, len(ids) - case.capacity)
            assert sorted(gid for _, _, gid in call.survivors) == [i for i in ids if i in store.buffer]
            assert [gid for _, _, gid in call.finished] == ids
            for i, game in enumerate(call.game_dicts):     # every finished game, survivor or not
                n = game["length"]
                assert game["id"] == ids[i] and n == got.length[i]
                assert np.array_equal(got.observations[i, : n + 1], game["observations"])
                assert np.array_equal(got.actions[i, : n + 1], game["actions"])
                assert np.array_equal(got.rewards[i, : n + 1].astype(np.float64), game["rewards"])
                assert np.array_equal(got.to_play[i, : n + 1], game["to_play"])
                assert got.child_visits[i, :n].tobytes() == game["child_visits"].tobytes()
                assert got.root_values[i, :n].tobytes() == game["root_values"].tobytes()
            synced += call.games
        assert rnd.running == filer.lengths().tolist()
        assert rnd.counters == store.counters()
        assert rnd.stored_ids == sorted(store.buffer)
        assert [rnd.env_index, rnd.length, rnd.ids] == [[g[i] for g in synced] for i in range(3)]
        for gid in rnd.stored_ids:
            game = rnd.slots[gid % case.capacity]
            assert game["id"] == gid == store.slot_id[gid % case.capacity] and game["length"] == store.buffer[gid]
            pri = ro.initial_priorities(rc.oracle_game(ro, game), case.td_steps, rc.DISCOUNT, 0.5)
            assert pri.dtype == np.float32 and pri.shape == (game["length"],) and np.isfinite(pri).all()
    filer.close()


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_every_case_reaches_its_condition(case):
    conditions = case.reaches(rc.run_model(case))
    for name, holds in conditions.items():
        print(f"{case.name}: {name}: {bool(holds)}")
    assert conditions and all(conditions.values()), {k: bool(v) for k, v in conditions.items()}


def names(cases):
    return [c.name for c in cases]


# mutation -> the cases that must notice it, and cases it must leave alone (so that a change is the rule's, not noise)
SENSITIVE = {
    "first_fit": (["block_edges_63", "block_edges_257", "calls_between_syncs"], ["block_edges_1"]),
    "dropped_off_by_one": (names(rc.WRAP), ["block_edges_63", "partial_eviction"]),
    "first_player": (names(rc.ACTION_WIDTHS), ["block_edges_63"]),
    "no_carry": (["scan_carry_1025", "scan_carry_2500", "scan_carry_2500_low_zero"], ["scan_carry_1023", "scan_carry_1024"]),
}


@pytest.mark.parametrize("mutation", rc.MUTATIONS)
def test_the_model_is_sensitive(mutation):
    by_name = {c.name: c for c in rc.CASES}
    notice, alone = SENSITIVE[mutation]
    for name in notice:
        assert rc.digest(rc.run_model(by_name[name], mutation)) != rc.digest(rc.run_model(by_name[name])), \
            f"the model with {mutation} says the same about {name}"
    for name in alone:
        assert rc.digest(rc.run_model(by_name[name], mutation)) == rc.digest(rc.run_model(by_name[name])), (mutation, name)


def test_the_model_is_deterministic():
    case = rc.BLOCK_EDGES[1]
    rc._TRACES.pop((case.name, None), None)
    first = rc.digest(rc.run_model(case))
    rc._TRACES.pop((case.name, None), None)
    assert rc.digest(rc.run_model(case)) == first
