"""K filers over one replay store: the model and the scenarios of tests/test_replay_filer_shared_cpu.py (CPU) and
tests/test_gpu_replay_filer_shared.py (the card).

The store numbers games in the order of the mzreplay_filer_file calls made on it, whatever stream each call runs on
(include/mzreplay.h).  Here are

  SharedModel    K FilerModels of tests/replay_filer_cases.py -- a running row per env, a list and an error word each --
                 over ONE store: the slot -> game and id -> length dicts are the same objects in all K, and the three
                 scalar counters are handed to the filer that files and taken back when its call returns.  The model's own
                 code runs unchanged; a refused call returns before it touches a counter;
  HostOrder      ReplayBuffer._add's bookkeeping game by game: the one host-order stream the K filers must equal;
  SCENARIOS      the named interleavings, each with the conditions it exists for as a predicate over its trace (`reaches`),
                 asserted on the CPU so that no case passes vacuously on the card.

The module imports no GPU code."""
import types

import numpy as np

import replay_filer_cases as rc


class SharedModel:
    def __init__(self, envs, max_moves, A, obs_shape, capacity, players, next_id=0):
        self.filers = [rc.FilerModel(E, max_moves, A, obs_shape, capacity, players, next_id) for E in envs]
        self.lengths_of, self.slots = self.filers[0].lengths_of, self.filers[0].slots
        for m in self.filers[1:]:
            m.lengths_of, m.slots = self.lengths_of, self.slots
        self.capacity, self.next_id, self.steps, self.total = capacity, next_id, 0, 0

    def file(self, k, batch):
        m = self.filers[k]
        m.next_id, m.steps, m.total = self.next_id, self.steps, self.total
        call = m.file(batch)
        self.next_id, self.steps, self.total = m.next_id, m.steps, m.total
        return call

    def counters(self):
        return [self.next_id, len(self.lengths_of), self.total, self.steps]

    def stored_ids(self):
        return sorted(self.lengths_of)


class HostOrder:
    """One store fed finished games one at a time, in the order they are handed to it (ReplayBuffer._add)."""

    def __init__(self, capacity, next_id=0):
        self.capacity, self.next_id, self.steps, self.total = capacity, next_id, 0, 0
        self.lengths_of, self.slots, self.slot_id = {}, {}, {}

    def add(self, games):
        """Returns (ids, ids evicted on the way that were stored before this add)."""
        ids, first, evicted_old = [], self.next_id, []
        for game in games:
            gid = self.next_id
            self.slots[gid % self.capacity], self.slot_id[gid % self.capacity] = game, gid
            self.lengths_of[gid] = game["length"]
            ids.append(gid)
            self.next_id += 1
            self.steps += game["length"]
            self.total += game["length"]
            if self.capacity < len(self.lengths_of):
                oldest = self.next_id - len(self.lengths_of)
                self.total -= self.lengths_of.pop(oldest)
                if oldest < first:
                    evicted_old.append(oldest)
        return ids, evicted_old

    def counters(self):
        return [self.next_id, len(self.lengths_of), self.total, self.steps]

    def slot_length(self):
        out = np.zeros(self.capacity, np.int32)
        for gid, n in self.lengths_of.items():
            out[gid % self.capacity] = n
        return out


class Scenario:
    """A store, K filers of envs[k] envs, and calls (k, spec) in the order the host makes them; one sync at the end (two
    for a filer whose first one reports a refusal)."""

    def __init__(self, name, envs, capacity, order, reaches, seed, M=4, max_moves=3, A=2, obs_shape=(1, 1, 3), players=1,
                 legal_form="per_move", td_steps=2, next_id=0):
        self.name, self.envs, self.capacity, self.order, self.reaches, self.seed = name, tuple(envs), capacity, order, reaches, seed
        self.M, self.max_moves, self.A, self.obs_shape, self.players = M, max_moves, A, tuple(obs_shape), players
        self.legal_form, self.td_steps, self.next_id = legal_form, td_steps, next_id
        self.E = max(envs)                                 # (what rc.config-style helpers read)

    def __repr__(self):
        return self.name


_TRACES = {}


def run_model(scn):
    """The scenario through SharedModel: the batches (for the card to file) and, per call, everything the store must
    show; at the end what every filer's sync hands out."""
    if scn.name in _TRACES:
        return _TRACES[scn.name]
    rs = np.random.RandomState(scn.seed)
    model = SharedModel(scn.envs, scn.max_moves, scn.A, scn.obs_shape, scn.capacity, scn.players, scn.next_id)
    first = []
    for k, E in enumerate(scn.envs):
        obs = rc.grid16(rs, (E,) + scn.obs_shape)
        tp = rs.randint(0, 2, E).astype(np.int32) if scn.players > 1 else None
        model.filers[k].begin(obs, tp)
        first.append((obs, tp))
    trace = types.SimpleNamespace(scenario=scn, first=first, steps=[])
    for k, spec in scn.order:
        spec = dict(spec)
        m = model.filers[k]
        before = model.counters()
        stored_before = model.stored_ids()
        slot_length = np.zeros(scn.capacity, np.int32)
        for gid, n in model.lengths_of.items():
            slot_length[gid % scn.capacity] = n
        running = m.len.copy()
        batch = rc.make_batch(rs, scn.envs[k], spec.pop("M", scn.M), scn.A, scn.obs_shape, scn.players, scn.legal_form,
                              running=m.len, max_moves=scn.max_moves, **spec)
        call = model.file(k, batch)
        trace.steps.append(types.SimpleNamespace(k=k, batch=batch, call=call, before=before, counters=model.counters(),
                                                 stored_before=stored_before, stored_ids=model.stored_ids(),
                                                 slot_length=slot_length, running_before=running,
                                                 slot_ids={s: g["id"] for s, g in model.slots.items()}))
    trace.syncs = []                                       # per filer: (error of the first sync, games handed out in the end)
    for m in model.filers:
        error, games = m.sync()
        if error is not None:
            _, games = m.sync()
        trace.syncs.append((error, games))
    trace.counters, trace.stored_ids, trace.slots = model.counters(), model.stored_ids(), dict(model.slots)
    trace.running = [m.len.tolist() for m in model.filers]
    _TRACES[scn.name] = trace
    return trace


def call(**kwargs):
    return dict(**kwargs)


def _calls_of(trace, k):
    return [s for s in trace.steps if s.k == k]


def reaches_two(first, second):
    """`first` files, `second` files in between its calls: A, B, A, B."""
    def reaches(trace):
        scn = trace.scenario
        steps = trace.steps
        other_evicted = any(s.call.refused is None and s.call.evicted_old > 0
                            and any(gid in {g[2] for t in steps[:i] if t.k != s.k for g in t.call.games}
                                    for gid in set(s.stored_before) - set(s.stored_ids))
                            for i, s in enumerate(steps))
        overflow_between = any(steps[i].call.n_new > scn.capacity and steps[i - 1].k == steps[i + 1].k != steps[i].k
                               and steps[i - 1].call.n_new > 0 and steps[i + 1].call.n_new > 0
                               for i in range(1, len(steps) - 1))
        return {"the calls alternate, starting with the named filer": [s.k for s in steps] == [first, second, first, second],
                "every call files games": all(s.call.n_new > 0 for s in steps),
                "a call evicts games the other filer stored": other_evicted,
                "a call finishes more games than slots between two calls of the other filer": overflow_between,
                "neither filer's ids are consecutive": all(
                    np.any(np.diff([g[2] for g in games]) > 1) for _, games in trace.syncs)}
    return reaches


def reaches_three(trace):
    steps = trace.steps
    return {"three filers file": {s.k for s in steps if s.call.n_new > 0} == {0, 1, 2},
            "a filer files twice in a row": any(a.k == b.k for a, b in zip(steps, steps[1:])),
            "the ring wraps": trace.counters[0] - trace.scenario.next_id > 2 * trace.scenario.capacity,
            "a non-zero first id": trace.scenario.next_id > 0,
            "games of all three are stored at the end": {k for k, (_, games) in enumerate(trace.syncs)
                                                         for g in games if g[2] in trace.stored_ids} == {0, 1, 2}}


def reaches_scan(trace):
    a, b = trace.steps
    return {"the first filer has filed": a.call.n_new > 0 and b.before[0] == trace.scenario.next_id + a.call.n_new,
            "a non-zero shared base for the second filer": b.call.first_id == b.before[0] > 0,
            "games by env 1023 and env 1024 in the second filer's call": rc.finished_by(b.call, rc.CHUNK - 1)
            and rc.finished_by(b.call, rc.CHUNK),
            "a non-zero carry into chunk 1": b.call.offsets[rc.CHUNK] > 0,
            "the last env finishes a game": rc.finished_by(b.call, trace.scenario.envs[1] - 1)}


def reaches_refusal(trace):
    steps = trace.steps
    bad = [i for i, s in enumerate(steps) if s.call.refused is not None]
    a_calls, b_calls = _calls_of(trace, 0), _calls_of(trace, 1)
    b_ids = [g[2] for s in b_calls[1:3] for g in s.call.games]
    return {"filer A's second call is refused for its legal set": len(a_calls) >= 2 and a_calls[0].call.refused is None
            and a_calls[0].call.n_new > 0 and a_calls[1].call.refused == rc.ERR_LEGAL,
            "a call of B right before and right after it": bool(bad) and steps[bad[0] - 1].k == 1 == steps[bad[0] + 1].k,
            "the refused call moves no counter": all(steps[i].before == steps[i].counters for i in bad),
            "B's ids stay contiguous across it": len(b_ids) > 2 and b_ids == list(range(b_ids[0], b_ids[0] + len(b_ids))),
            "every call of B files": all(s.call.refused is None and s.call.n_new > 0 for s in b_calls),
            "A's later unsynced call is refused with it": len(a_calls) == 3 and a_calls[2].call.refused == rc.ERR_LEGAL
            and max(a_calls[2].call.played) > 0,
            "A's first sync reports it, the next hands out its first call's games": trace.syncs[0][0] == rc.ERR_LEGAL
            and trace.syncs[0][1] == a_calls[0].call.games,
            "B's sync reports nothing": trace.syncs[1][0] is None}


A, B, C = 0, 1, 2
FULL = call(stall_rate=0.0, done_rate=0.5)
ORDER_AB = Scenario("order_A_B_A_B", (3, 5), 4, [(A, FULL), (B, FULL), (A, FULL), (B, FULL)], reaches_two(A, B), seed=2901)
ORDER_BA = Scenario("order_B_A_B_A", (3, 5), 4, [(B, FULL), (A, FULL), (B, FULL), (A, FULL)], reaches_two(B, A), seed=2902)
THREE = Scenario("three_filers", (4, 2, 6), 7, [(A, call()), (B, call()), (C, call()), (B, call(M=2)), (A, call()), (C, call(M=5)),
                                               (C, call()), (B, call(M=1, stall_rate=0.0, finish=(0,))),
                                               (A, call(M=1, stall_rate=0.0, finish=(1,)))], reaches_three, seed=2903,
                 players=2, legal_form="wide", A=3, next_id=12345)
SCAN_BASE = Scenario("scan_carry_on_a_shared_base", (6, 1030), 4096,
                     [(A, FULL), (B, call(finish=(rc.CHUNK - 1, rc.CHUNK, 1029)))], reaches_scan, seed=2904, M=3, next_id=77)
GOOD = call(M=2, stall_rate=0.0, done_rate=0.6)
REFUSAL = Scenario("a_refusal_stays_with_its_filer", (5, 4), 32,
                   [(B, GOOD), (A, GOOD), (B, GOOD), (A, call(M=2, stall_rate=0.0, corrupt=(1, 3))), (B, GOOD), (A, GOOD), (B, GOOD)],
                   reaches_refusal, seed=2905)
SCENARIOS = [ORDER_AB, ORDER_BA, THREE, SCAN_BASE, REFUSAL]
