"""Several filers into one replay store (include/mzreplay.h: the store numbers games in the order of the
mzreplay_filer_file calls made on it), on the CPU:

* the numpy model of tests/replay_filer_cases.py driven as K filers over one store (tests/replay_filer_shared_cases.py),
  calls interleaved in a given order, against the same finished games fed through ONE host-order stream
  (ReplayBuffer._add's bookkeeping): ids, slots, evictions and the four counters after every call;
* csrc/replay_filer.h itself, built with g++ (tests/replay_filer_check.cpp, as tests/test_replay_filer_cpu.py builds it),
  given every call's shared counters and the calling filer's own running lengths: a call that evicts another filer's
  games needs no new case in evicted_old / first_evicted_id;
* every scenario reaches the conditions it is named for (the card runs the same scenarios);
* the C ABI of mzreplay_filer_sync_ids: declared, exported, bound with seven arguments, null arguments refused.

mzreplay_filer_sync's message on a store with two filers needs a store, which needs a device: it is asserted on the card
(tests/test_gpu_replay_filer_shared.py)."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import replay_filer_cases as rc
import replay_filer_shared_cases as sc
from test_replay_filer_cpu import check   # noqa: F401  (the fixture that builds tests/replay_filer_check.cpp)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_game(a, b):
    return a["length"] == b["length"] and all(np.ascontiguousarray(a[key]).tobytes() == np.ascontiguousarray(b[key]).tobytes()
                                              for key in rc.ARRAYS[1:])


@pytest.mark.parametrize("scn", sc.SCENARIOS, ids=repr)
def test_k_filers_over_one_store_equal_one_host_order_stream(scn):
    trace = sc.run_model(scn)
    host = sc.HostOrder(scn.capacity, scn.next_id)
    for i, step in enumerate(trace.steps):
        where = f"{scn.name} call {i} (filer {step.k})"
        assert step.before == host.counters(), where
        if step.call.refused is not None:                  # nothing is handed to the host path, and nothing moved
            assert step.counters == step.before and step.stored_ids == step.stored_before and step.call.games == [], where
            continue
        ids, evicted_old = host.add(step.call.game_dicts)
        assert [g[2] for g in step.call.games] == ids and step.call.first_id == step.before[0], where
        assert [g[1] for g in step.call.games] == [g["length"] for g in step.call.game_dicts], where
        assert step.counters == host.counters(), where
        assert step.stored_ids == sorted(host.lengths_of), where
        assert sorted(set(step.stored_before) - set(step.stored_ids)) == evicted_old, where
        assert step.call.evicted_old == len(evicted_old), where
        if evicted_old:
            assert step.call.first_evicted_id == evicted_old[0], where
        assert step.slot_ids == host.slot_id, where
    assert trace.counters == host.counters()
    assert sorted(trace.slots) == sorted(host.slots)
    for slot, game in trace.slots.items():
        assert game["id"] == host.slot_id[slot] and same_game(game, host.slots[slot]), f"{scn.name}: slot {slot}"
    # what the filers' syncs hand out: each filer's own games, ids ascending, all of them together every id once
    handed = sorted(g[2] for _, games in trace.syncs for g in games)
    filed = sorted(g[2] for s in trace.steps for g in s.call.games)
    assert handed == filed == list(range(scn.next_id, scn.next_id + len(filed)))
    for k, (_, games) in enumerate(trace.syncs):
        assert games == [g for s in trace.steps if s.k == k for g in s.call.games]


@pytest.mark.parametrize("scn", sc.SCENARIOS, ids=repr)
def test_every_scenario_reaches_what_it_is_named_for(scn):
    missed = [what for what, reached in scn.reaches(sc.run_model(scn)).items() if not reached]
    assert not missed, f"{scn.name} does not reach: {missed}"


def test_the_scenarios_cover_two_and_three_filers_and_a_four_slot_store():
    assert {len(s.envs) for s in sc.SCENARIOS} == {2, 3}
    assert any(s.capacity == 4 for s in sc.SCENARIOS)


@pytest.mark.parametrize("scn", sc.SCENARIOS, ids=repr)
def test_the_header_arithmetic_on_shared_counters(check, scn):   # noqa: F811
    """csrc/replay_filer.h per call: `before` is the store's, the running lengths the calling filer's."""
    trace = sc.run_model(scn)
    for i, step in enumerate(trace.steps):
        if step.call.refused is not None:                  # (a bad legal set: the check program is given no legal sets)
            continue
        b = step.batch
        got = check(step.call.E, step.call.M, scn.capacity, scn.max_moves, rc.CHUNK, step.before, step.running_before,
                    step.slot_length, b["actions"], b["done"])
        where = f"{scn.name} call {i} (filer {step.k})"
        assert got["refused"] == 0, where
        assert got["env"] == [g[0] for g in step.call.games], where
        assert got["length"] == [g[1] for g in step.call.games], where
        assert got["id"] == [g[2] for g in step.call.games], where
        assert got["slot"] == [g[2] % scn.capacity for g in step.call.games], where
        assert got["counters"] == step.counters, where


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_sync_ids_is_declared_exported_and_bound(pkg):
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mzreplay.h")).read(), flags=re.S)
    declared = re.search(r"\bint\s+mzreplay_filer_sync_ids\s*\(([^)]*)\)", text)
    assert declared, "mzreplay_filer_sync_ids is not declared"
    arguments = [" ".join(a.split()) for a in declared.group(1).split(",")]
    assert arguments == ["mzreplay_filer *filer", "int32_t *n_new", "const int32_t **env_index", "const int32_t **lengths",
                         "const int64_t **game_ids", "int64_t *counters", "void *stream"]
    assert hasattr(lib, "mzreplay_filer_sync_ids"), "mzreplay_filer_sync_ids is not exported"
    restype, argtypes = native.PROTOTYPES["mzreplay_filer_sync_ids"]
    assert restype is ctypes.c_int and len(argtypes) == len(arguments)
    # mzreplay_filer_sync keeps its signature
    kept = re.search(r"\bint\s+mzreplay_filer_sync\s*\(([^)]*)\)", text)
    assert [" ".join(a.split()) for a in kept.group(1).split(",")] == [
        "mzreplay_filer *filer", "int32_t *n_new", "const int32_t **env_index", "const int32_t **lengths",
        "int64_t *first_game_id", "int64_t *counters", "void *stream"]
    assert len(native.PROTOTYPES["mzreplay_filer_sync"][1]) == 7


def test_sync_ids_refuses_null_arguments_with_a_message(pkg):
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    n = ctypes.c_int32()
    assert lib.mzreplay_filer_sync_ids(None, ctypes.byref(n), None, None, None, None, None) != 0
    assert b"mzreplay_filer_sync" in lib.mzreplay_last_error(None)


def test_the_header_states_the_ordering_rule():
    text = " ".join(open(os.path.join(ROOT, "include", "mzreplay.h")).read().replace(" * ", " ").split())
    assert "one per store" not in text
    assert "in the order of the mzreplay_filer_file calls made on it" in text


def test_python_surface_of_several_filers(pkg):
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    rb = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    for name in ("begin", "file", "lengths", "take_filed"):
        assert hasattr(rb.DeviceFiler, name)
    assert isinstance(rb.ReplayBuffer.filers, property)
    # joining a store that already has a filing actor is an explicit request, for one actor and for the pipelined one
    for cls in (sp.DeviceSelfPlay, sp.PipelinedDeviceSelfPlay):
        assert inspect.signature(cls.file_to).parameters["shared"].default is False
    # and the sink is a ReplayBuffer's device store, nothing else
    with pytest.raises(NotImplementedError, match="ReplayBuffer"):
        sp.PipelinedDeviceSelfPlay.file_to(object.__new__(sp.PipelinedDeviceSelfPlay), object())
