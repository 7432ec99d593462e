"""Inputs and the model of the replay-filer tests (test_gpu_replay_filer_forms.py on the card,
test_replay_filer_reference.py on the CPU).

The device filer (include/mzreplay.h mzreplay_filer_*, kernels in csrc/mzreplay.hip) turns a move batch, read where the
search engine and the environment kernels left it, into stored games.  Here are

  make_batch     a seeded move batch in the ring layout of mzreplay_file_moves, with values that cannot hide an error:
                 S = 7 simulations (visits / S and root_value_sum / S are inexact fp64 divisions), float32 normal rewards,
                 observations on a 1/16 grid that differ in obs_after and obs_next, players drawn per move, legal sets that
                 are permuted subsets, and GARBAGE in every visit and legal entry past n_legal;
  FilerModel     rules 1-5 of include/mzreplay.h one move at a time in plain numpy: a running row per env, a dict slot ->
                 game, the four counters moved "as if all had been stored and evicted in turn";
  CASES          the named shapes, each with the condition it exists for as a predicate over the model's trace
                 (`reaches`): a case whose seed stops reaching its edge fails on the CPU, not vacuously on the card;
  upload / file_moves / misaligned
                 a batch as device tensors behind a _native.MzReplayFileMoves.

The module imports no GPU code; the upload helpers ask for torch when they are called."""
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7                     # num_simulations: no visit count or value sum divides exactly
GARBAGE = 0x7F7F7F7F      # in visits / legal entries past n_legal: never to be read, least of all as an index
CHUNK = 1024              # counts filer_scan_kernel scans at a time (kScanThreads)
BLOCK = 256               # envs per workgroup of filer_count_kernel
GRID = 2048               # workgroups filer_priorities_kernel has at the most
DISCOUNT = 0.997          # of every case's store
ERR_LEGAL = "mzhist_file: a legal-action count outside"
ERR_OVERFLOW = "mzhist_file: a game outgrew max_moves"
ARRAYS = ("length", "observations", "actions", "rewards", "to_play", "child_visits", "root_values")
MUTATIONS = ("first_fit", "dropped_off_by_one", "first_player", "no_carry")


def replay_oracle():
    path = os.path.join(ROOT, "oracle")
    if path not in sys.path:
        sys.path.insert(0, path)
    import replay_oracle as ro
    return ro


# ---- batches ----------------------------------------------------------------------------------------------------------
def grid16(rs, shape):
    return (np.round(rs.standard_normal(shape) * 16) / 16).astype(np.float32)


def make_batch(rs, E, M, A, obs_shape, players, legal_form, running=None, max_moves=None, stall_rate=0.3, done_rate=0.4,
               stall_at_zero=(), finish=(), quiet=(), unforced=(), corrupt=None):
    """A move batch as numpy arrays in the ring layout: actions i32[M, E] (-1 from an env's stall move onwards), visits
    i32[M, E, A], root_value_sum f64[M, E], legal / num_legal (per move [M, E, A] / [M, E]; legal_form "batch": one set per
    env for the whole batch, [E, A] / [E], read with stride 0), to_play i32[M, E] and to_play_last i32[E] (None for one
    player), rewards f32[M, E], done u8[M, E], obs_after / obs_next f32[M, E, ...].

    running / max_moves: a done flag is forced where an env's running length reaches max_moves (not for the envs in
    `unforced`: the overflow case).  stall_at_zero: envs that play nothing; finish: envs that play the whole batch and end
    a game on its first move; quiet: envs without seeded done flags.  legal_form: "per_move" (n_legal uniform in 0..A),
    "wide" (n_legal from {0, 1, A, uniform}), "batch".  corrupt = (m, e): that move's first legal action reads A."""
    running = np.zeros(E, np.int64) if running is None else np.asarray(running, np.int64)
    stall = np.full(E, M, np.int64)
    stalls = rs.random_sample(E) < stall_rate
    stall[stalls] = rs.randint(0, M, int(stalls.sum()))            # a stall at move 0 included
    stall[list(stall_at_zero)] = 0
    stall[list(finish)] = M
    actions = rs.randint(0, A, (M, E)).astype(np.int32)
    for e in range(E):
        actions[stall[e]:, e] = -1
    done = (rs.random_sample((M, E)) < done_rate).astype(np.uint8)
    done[:, list(quiet)] = 0
    done[0, list(finish)] = 1
    length = running.copy()
    for m in range(M):
        for e in range(E):
            if m >= stall[e]:
                continue                                           # (flags past the prefix stay as drawn: never read)
            length[e] += 1
            if max_moves is not None and length[e] >= max_moves and e not in unforced:
                done[m, e] = 1
            if done[m, e]:
                length[e] = 0
    per_env = legal_form == "batch"
    rows = E if per_env else M * E
    legal = np.full((rows, A), GARBAGE, np.int32)
    num_legal = np.zeros(rows, np.int32)
    visits = np.full((M * E, A), GARBAGE, np.int32)
    for r in range(rows):
        if legal_form == "wide":
            n = int(rs.choice([0, 1, A, rs.randint(0, A + 1)]))
        elif per_env:
            n = int(rs.randint(1, A + 1))
        else:
            n = int(rs.randint(0, A + 1))
        num_legal[r] = n
        legal[r, :n] = rs.permutation(A)[:n]
    for r in range(M * E):
        n = int(num_legal[r % E if per_env else r])
        if n:
            visits[r, :n] = rs.multinomial(S, rs.dirichlet([0.6] * n))
    batch = dict(actions=actions, visits=visits.reshape(M, E, A), root_value_sum=rs.standard_normal((M, E)) * S,
                 legal=legal if per_env else legal.reshape(M, E, A), num_legal=num_legal if per_env else num_legal.reshape(M, E),
                 to_play=None, to_play_last=None, rewards=rs.standard_normal((M, E)).astype(np.float32), done=done,
                 obs_after=grid16(rs, (M, E) + tuple(obs_shape)), obs_next=grid16(rs, (M, E) + tuple(obs_shape)),
                 players=players)
    if players > 1:
        batch["to_play"] = rs.randint(0, 2, (M, E)).astype(np.int32)           # drawn per move: not alternating
        batch["to_play_last"] = rs.randint(0, 2, E).astype(np.int32)           # and independently
    if corrupt is not None:
        m, e = corrupt
        assert not per_env and actions[m, e] >= 0
        batch["num_legal"][m, e] = max(1, batch["num_legal"][m, e])
        batch["legal"][m, e, 0] = A
    return batch


# ---- the model --------------------------------------------------------------------------------------------------------
class FilerModel:
    """The filer's contract (include/mzreplay.h, rules 1-5) one move at a time.  obs / act / rew / tp / cv / rv / len are
    the running games, a row per env; `slots` maps slot -> stored game (a dict of the seven arrays over the game's own
    extent, plus its id), `lengths_of` id -> length of every game the counters call stored.  A refusal stands until the
    sync that reports it: calls in between are refused with it.  `mutation` breaks one rule on purpose
    (test_replay_filer_reference.py)."""

    def __init__(self, E, max_moves, A, obs_shape, capacity, players, next_id=0, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.E, self.L, self.A, self.capacity, self.players, self.mutation = E, max_moves, A, capacity, players, mutation
        self.obs = np.zeros((E, max_moves + 1) + tuple(obs_shape), np.float32)
        self.act = np.zeros((E, max_moves + 1), np.int32)
        self.rew = np.zeros((E, max_moves + 1), np.float64)
        self.tp = np.zeros((E, max_moves + 1), np.int32)
        self.cv = np.zeros((E, max_moves, A), np.float64)
        self.rv = np.zeros((E, max_moves), np.float64)
        self.len = np.zeros(E, np.int64)
        self.next_id, self.steps, self.total = next_id, 0, 0
        self.lengths_of, self.slots = {}, {}
        self.error = None                  # the device error word, as its message
        self.pending = []                  # (env, length, id) of the games filed since the last sync

    def begin(self, first_obs, first_to_play=None):
        for e in range(self.E):
            self.obs[e, 0] = first_obs[e]
            self.act[e, 0], self.rew[e, 0], self.len[e] = 0, 0.0, 0
            self.tp[e, 0] = 0 if first_to_play is None else first_to_play[e]

    def counters(self):
        return [self.next_id, len(self.lengths_of), self.total, self.steps]

    def stored_ids(self):
        return sorted(self.lengths_of)

    def game(self, gid):
        game = self.slots[gid % self.capacity]
        assert game["id"] == gid, f"slot {gid % self.capacity} holds game {game['id']}, not {gid}"
        return game

    def _legal(self, b, m, e):
        if b["legal"].ndim == 3:
            return int(b["num_legal"][m, e]), b["legal"][m, e]
        return int(b["num_legal"][e]), b["legal"][e]

    def file(self, b):
        """One mzreplay_filer_file.  Returns a record of the call: what the kernels' plan holds, and `games` = the
        (env_index, length, id) the call adds to the next sync's list."""
        E, M = self.E, b["actions"].shape[0]
        call = types.SimpleNamespace(E=E, M=M, refused=None, played=[0] * E, counts=[0] * E, offsets=[0] * E, n_new=0,
                                     dropped=0, first_id=self.next_id, stored_before=len(self.lengths_of), evicted_old=0,
                                     first_evicted_id=self.next_id - len(self.lengths_of), games=[], running_before=self.len.copy())
        # rule 2: the played moves are a prefix; rule 5: everything is checked before anything is used
        bad_legal = overflow = False
        for e in range(E):
            k = 0
            while k < M and b["actions"][k, e] >= 0:
                k += 1
            call.played[e] = k
            n = int(self.len[e])
            for m in range(k):
                n_legal, legal = self._legal(b, m, e)
                if n_legal < 0 or n_legal > self.A:
                    bad_legal = True
                else:
                    for i in range(n_legal):
                        if legal[i] < 0 or legal[i] >= self.A:
                            bad_legal = True
                n += 1
                if n > self.L:
                    overflow = True
                if b["done"][m, e]:
                    n = 0
        if bad_legal and self.error is None:
            self.error = ERR_LEGAL
        elif overflow and self.error is None:
            self.error = ERR_OVERFLOW
        if self.error is not None:         # this call's, or an earlier one's the sync has not reported yet
            call.refused = self.error
            return call
        # rule 1: the moves, one at a time
        finished = []                      # (env, move, game), env-major then in move order
        for e in range(E):
            for m in range(call.played[e]):
                at = int(self.len[e])
                n_legal, legal = self._legal(b, m, e)
                self.cv[e, at] = 0.0
                for i in range(n_legal):
                    self.cv[e, at, legal[i]] = float(b["visits"][m, e, i]) / float(S)
                self.rv[e, at] = float(b["root_value_sum"][m, e]) / float(S)
                self.act[e, at + 1] = b["actions"][m, e]
                self.rew[e, at + 1] = float(b["rewards"][m, e])
                self.obs[e, at + 1] = b["obs_after"][m, e]
                to_play = 0 if b["to_play"] is None else int(b["to_play"][m, e])
                self.tp[e, at + 1] = 1 - to_play if self.players > 1 else 0
                self.len[e] = n = at + 1
                if b["done"][m, e]:
                    finished.append((e, m, dict(length=n, observations=self.obs[e, : n + 1].copy(), actions=self.act[e, : n + 1].copy(),
                                                rewards=self.rew[e, : n + 1].copy(), to_play=self.tp[e, : n + 1].copy(),
                                                child_visits=self.cv[e, :n].copy(), root_values=self.rv[e, :n].copy())))
                    call.counts[e] += 1
                    self.len[e] = 0
                    self.obs[e, 0] = b["obs_next"][m, e]
                    self.act[e, 0], self.rew[e, 0] = 0, 0.0
                    following = 0          # the next move's recorded player: the envs' own after the batch's last move
                    if b["to_play"] is not None:
                        following = int(b["to_play"][m + 1, e]) if m + 1 < M else int(b["to_play_last"][e])
                        if self.mutation == "first_player":
                            following = 1 - to_play
                    self.tp[e, 0] = following
        # rule 3: env-major ranks, the exclusive scan over E taken a chunk at a time with the total carried along
        carry = 0
        for base in range(0, E, CHUNK):
            run = 0 if self.mutation == "no_carry" else carry
            for e in range(base, min(base + CHUNK, E)):
                call.offsets[e] = run
                run += call.counts[e]
            carry = carry + run if self.mutation == "no_carry" else run
        call.n_new = n_new = len(finished)
        assert carry == n_new
        rank_in_env, ranked = {}, []
        for e, m, game in finished:
            r = rank_in_env.get(e, 0)
            rank_in_env[e] = r + 1
            ranked.append((call.offsets[e] + r, e, m, game))
        if self.mutation == "first_fit":   # numbered as they finish in time
            ranked = [(j, e, m, game) for j, (e, m, game) in enumerate(sorted(finished, key=lambda f: (f[1], f[0])))]
        ranked.sort(key=lambda item: item[0])
        # rule 4: only the last `capacity` games of a call are written; the counters move as if all had been stored and
        # evicted in turn (ReplayBuffer._add, game by game)
        call.dropped = n_new - self.capacity if n_new > self.capacity else 0
        if self.mutation == "dropped_off_by_one" and call.dropped:
            call.dropped += 1
        first = self.next_id
        for j, e, m, game in ranked:
            gid = first + j
            game["id"] = gid
            survived = j >= call.dropped
            if survived:
                self.slots[gid % self.capacity] = game
            self.lengths_of[gid] = game["length"]
            self.next_id += 1
            self.steps += game["length"]
            self.total += game["length"]
            if self.capacity < len(self.lengths_of):
                oldest = self.next_id - len(self.lengths_of)
                if oldest < first:
                    call.evicted_old += 1
                self.total -= self.lengths_of.pop(oldest, 0)
            call.games.append((e, game["length"], gid))
            self.pending.append((e, game["length"], gid))
        call.survivors = [(e, m, gid) for j, e, m, game in ranked if j >= call.dropped for gid in [first + j]]
        call.finished = [(e, m, first + j) for j, e, m, game in ranked]
        call.game_dicts = [game for _, _, _, game in ranked]       # every finished game, dropped ones included
        return call

    def sync(self):
        """One mzreplay_filer_sync: the error word's message (and the list kept for the next sync), or the list."""
        if self.error is not None:
            message, self.error = self.error, None
            return message, []
        games, self.pending = self.pending, []
        return None, games


# ---- cases ------------------------------------------------------------------------------------------------------------
def call(M=3, **kwargs):
    return dict(M=M, **kwargs)


class Case:
    """A store, an actor of E envs and rounds of calls, each round closed by a sync."""

    def __init__(self, name, E, capacity, rounds, reaches, seed=0, max_moves=3, A=2, obs_shape=(1, 1, 3), players=1,
                 legal_form="per_move", td_steps=2, next_id=0, twin=False, misalign=(), small=True):
        self.name, self.E, self.capacity, self.rounds, self.reaches, self.seed = name, E, capacity, rounds, reaches, seed
        self.max_moves, self.A, self.obs_shape, self.players, self.legal_form = max_moves, A, tuple(obs_shape), players, legal_form
        self.td_steps, self.next_id, self.twin, self.misalign, self.small = td_steps, next_id, twin, tuple(misalign), small

    @property
    def obs_floats(self):
        return int(np.prod(self.obs_shape))

    def __repr__(self):
        return self.name


_TRACES = {}


def run_model(case, mutation=None):
    """The case through the model: the batches (for the card to file) and, per round, everything a sync must show."""
    key = (case.name, mutation)
    if key in _TRACES:
        return _TRACES[key]
    rs = np.random.RandomState(case.seed)
    model = FilerModel(case.E, case.max_moves, case.A, case.obs_shape, case.capacity, case.players, case.next_id, mutation)
    first_obs = grid16(rs, (case.E,) + case.obs_shape)
    first_tp = rs.randint(0, 2, case.E).astype(np.int32) if case.players > 1 else None
    model.begin(first_obs, first_tp)
    trace = types.SimpleNamespace(case=case, first_obs=first_obs, first_to_play=first_tp, rounds=[])
    for specs in case.rounds:
        rnd = types.SimpleNamespace(batches=[], calls=[])
        for spec in specs:
            spec = dict(spec)
            batch = make_batch(rs, case.E, spec.pop("M"), case.A, case.obs_shape, case.players, case.legal_form,
                               running=model.len, max_moves=case.max_moves, **spec)
            rnd.batches.append(batch)
            rnd.calls.append(model.file(batch))
        rnd.error, games = model.sync()
        if rnd.error is not None:          # the following sync hands out what the calls before the refused one filed
            _, games = model.sync()
        rnd.env_index, rnd.length, rnd.ids = ([g[i] for g in games] for i in range(3))
        rnd.counters, rnd.stored_ids, rnd.running = model.counters(), model.stored_ids(), model.len.tolist()
        rnd.slots = dict(model.slots)      # (a stored game's dict is never written again)
        trace.rounds.append(rnd)
    _TRACES[key] = trace
    return trace


def digest(trace):
    """Everything the model says about a case, as one hash."""
    h = hashlib.sha256()
    for rnd in trace.rounds:
        h.update(repr((rnd.error, rnd.env_index, rnd.length, rnd.ids, rnd.counters, rnd.stored_ids, rnd.running)).encode())
        for slot in sorted(rnd.slots):
            game = rnd.slots[slot]
            h.update(repr((slot, game["id"], game["length"])).encode())
            for key in ARRAYS[1:]:
                h.update(np.ascontiguousarray(game[key]).tobytes())
    return h.hexdigest()


def padded_games(case, games):
    """Games (the model's dicts) as arrays in mzreplay_add_games' layout: rows max_moves wide, zero past each extent."""
    G, L = len(games), case.max_moves
    out = dict(lengths=np.array([g["length"] for g in games], np.int32),
               observations=np.zeros((G, L + 1) + case.obs_shape, np.float32), actions=np.zeros((G, L + 1), np.int32),
               rewards=np.zeros((G, L + 1), np.float64), to_play=np.zeros((G, L + 1), np.int32),
               child_visits=np.zeros((G, L, case.A), np.float64), root_values=np.zeros((G, L), np.float64))
    for g, game in enumerate(games):
        n = game["length"]
        for key in ARRAYS[1:]:
            out[key][g, : len(game[key])] = game[key]
        assert len(game["observations"]) == n + 1 and len(game["child_visits"]) == n
    return out


def oracle_game(ro, game):
    """The model's game as the oracle's Game (cached on the dict), its initial priorities not yet computed."""
    if "oracle" not in game:
        game["oracle"] = ro.Game(game["observations"], game["actions"], game["rewards"], game["to_play"],
                                 game["child_visits"], game["root_values"])
    return game["oracle"]


def all_calls(trace):
    return [c for rnd in trace.rounds for c in rnd.calls]


def finished_by(call_record, env):
    return any(e == env for e, _, _ in call_record.finished)


def straddles(c):
    """An env whose first game of the call is dropped and whose second survives."""
    first = c.first_id
    by_env = {}
    for e, m, gid in c.finished:
        by_env.setdefault(e, []).append(gid - first)
    return any(len(r) >= 2 and r[0] < c.dropped <= r[1] for r in by_env.values())


def reaches_block_edges(E):
    def reaches(trace):
        calls = all_calls(trace)
        out = {"the last env finishes a game": any(finished_by(c, E - 1) for c in calls),
               "blocks of 256 envs": (E + BLOCK - 1) // BLOCK == {1: 1, 63: 1, 255: 1, 256: 1, 257: 2}[E]}
        if E > BLOCK:
            out["the last env of a block and the first of the next finish a game in one call"] = any(
                finished_by(c, BLOCK - 1) and finished_by(c, BLOCK) for c in calls)
        return out
    return reaches


def reaches_scan(E, variant):
    def reaches(trace):
        calls = all_calls(trace)
        out = {"two calls": len(calls) == 2 and all(c.n_new > 0 for c in calls)}
        if variant == "plain":
            out["the last env finishes a game"] = any(finished_by(c, E - 1) for c in calls)
            if E > CHUNK:
                out["games by env 1023 and env 1024 in one call"] = any(finished_by(c, CHUNK - 1) and finished_by(c, CHUNK) for c in calls)
                out["a non-zero carry into chunk 1"] = all(c.offsets[CHUNK] > 0 for c in calls)
        if variant == "low_zero":
            out["every count of envs 0..1023 is zero"] = all(not any(c.counts[:CHUNK]) for c in calls)
            out["games in envs >= 1024"] = all(sum(c.counts[CHUNK:]) > 0 for c in calls)
            out["a zero carry into chunk 1, a non-zero one into chunk 2"] = all(
                c.offsets[CHUNK] == 0 and c.offsets[2 * CHUNK] > 0 and sum(c.counts[2 * CHUNK:]) > 0 for c in calls)
        if variant == "high_zero":
            out["every count of envs >= 1024 is zero"] = all(not any(c.counts[CHUNK:]) for c in calls)
            out["a non-zero carry over chunks of zeros"] = all(c.offsets[CHUNK] > 0 and c.offsets[E - 1] == c.n_new for c in calls)
        return out
    return reaches


def reaches_wrap(capacity):
    def reaches(trace):
        pre, c = trace.rounds[0].calls[0], trace.rounds[1].calls[0]
        slots = [gid % capacity for _, _, gid in c.finished]
        return {"the store is pre-filled by an earlier call": pre.n_new > 0 and c.stored_before == min(pre.n_new, capacity),
                "dropped > 1024": c.dropped > CHUNK,
                "an env whose first game of the call is dropped and whose second survives": straddles(c),
                "two new games of the call would share a slot without the drop rule": len(set(slots)) < len(slots),
                "the survivors take every slot once": sorted(gid % capacity for _, _, gid in c.survivors) == list(range(capacity))}
    return reaches


def reaches_partial_eviction(trace):
    case, c = trace.case, trace.rounds[1].calls[0]
    at = c.first_evicted_id % case.capacity
    return {"evicted_old in (1024, games_stored)": CHUNK < c.evicted_old < c.stored_before,
            "first_evicted_id % G near G": case.capacity - 64 <= at < case.capacity,
            "the slot walk crosses the ring's end": at + c.evicted_old > case.capacity,
            "more than 2048 surviving games in a call": len(c.survivors) > GRID and c.dropped == 0}


def reaches_long_game(trace):
    ro, case = replay_oracle(), trace.case
    long_games = [g for g in trace.rounds[-1].slots.values() if g["length"] > 256]
    tails, late_max = [], False
    for game in long_games:
        pri = ro.initial_priorities(oracle_game(ro, game), case.td_steps, DISCOUNT, 0.5)
        tails.append(bool((pri[256:] > 0).all()))
        late_max |= int(np.argmax(pri)) >= 256
    return {"a game of more than 256 moves": bool(long_games),
            "carried across calls in the running row": any(g["length"] > c.M for g in long_games for c in all_calls(trace)),
            "positions >= 256 have non-zero priority": bool(tails) and all(tails),
            "a game's maximum lies at a position >= 256": late_max,
            "short games beside it": any(g["length"] < 20 for g in trace.rounds[-1].slots.values())}


def reaches_action_widths(A):
    def reaches(trace):
        seen, permuted, not_alternating, last_move = set(), False, False, False
        for rnd in trace.rounds:
            for b, c in zip(rnd.batches, rnd.calls):
                for e in range(c.E):
                    for m in range(c.played[e]):
                        n = int(b["num_legal"][m, e])
                        seen.add(n)
                        permuted |= n > 1 and b["legal"][m, e, :n].tolist() != sorted(b["legal"][m, e, :n].tolist())
                        if m + 1 < c.played[e]:
                            not_alternating |= b["to_play"][m + 1, e] == b["to_play"][m, e]
                for e, m, _ in c.finished:
                    last_move |= m == c.M - 1 and b["to_play_last"][e] != 1 - b["to_play"][m, e]
        out = {"n_legal = 0, 1 and A all occur": {0, 1, A} <= seen,
               "to_play does not alternate": bool(not_alternating),
               "a game ends on the batch's last move with to_play_last != 1 - to_play": bool(last_move)}
        if A > 1:
            out["a legal set that is a non-identity permutation"] = bool(permuted)
        if A > 64:
            out["a policy row wider than the wavefront"] = True
        return out
    return reaches


def reaches_one_legal_set(trace):
    b = trace.rounds[0].batches[0]
    return {"one legal set per env for the batch": b["legal"].ndim == 2 and b["num_legal"].ndim == 1,
            "games are filed": all(c.n_new > 0 for c in all_calls(trace)),
            "sets of one and of two actions": set(b["num_legal"].tolist()) == {1, 2}}


def takes_vec4(obs_floats, obs_after_ptr, obs_next_ptr):
    """mzreplay_filer_file's rule for the 16-byte copy path."""
    return obs_floats % 4 == 0 and obs_after_ptr % 16 == 0 and obs_next_ptr % 16 == 0


def reaches_obs(trace):
    case = trace.case
    out = {"games are filed in both calls": all(c.n_new > 0 for c in all_calls(trace)),
           "a game of several moves": any(n > 1 for rnd in trace.rounds for n in rnd.length)}
    # (pointer alignment is the card's to show; test_gpu_replay_filer_forms.py asserts the path from the real pointers)
    out["the path the host must choose"] = takes_vec4(case.obs_floats, 0, 0) == (case.obs_floats % 4 == 0)
    if case.obs_floats == 260:
        out["65 float4 > 64 lanes"] = case.obs_floats // 4 > 64
    return out


def list_plan(E, sizes):
    """The host's list handling in mzreplay_filer_file, restated: per call (drained, grown)."""
    cap = bound = 0
    out = []
    for M in sizes:
        most = E * M
        drained = grown = False
        if bound + most > cap:
            drained, bound = True, 0
            if most > cap:
                grown, cap = True, most
        bound += most
        out.append((drained, grown))
    return out


def reaches_between_syncs(trace):
    rnd = trace.rounds[0]
    plan = list_plan(trace.case.E, [c.M for c in rnd.calls])
    return {"three calls, one sync": len(rnd.calls) == 3 and len(trace.rounds) == 1,
            "the second call takes the drain without growing": plan[1] == (True, False),
            "the third call grows the list": plan[2] == (True, True),
            "every call files games": all(c.n_new > 0 for c in rnd.calls),
            "ids consecutive across the three": rnd.ids == list(range(rnd.ids[0], rnd.ids[0] + len(rnd.ids)))
            and len(rnd.ids) == sum(c.n_new for c in rnd.calls)}


def reaches_reanalysed(trace):
    first, second = trace.rounds[0], trace.rounds[1]
    return {"four stored games that bootstrap": first.stored_ids == [0, 1, 2, 3] and all(n == 3 for n in first.length),
            "the second call overwrites two of the four slots": second.ids == [4, 5] and second.stored_ids == [2, 3, 4, 5],
            "the new games bootstrap too": all(n == 3 for n in second.length)}


def reaches_overflow(trace):
    one, two, three = trace.rounds
    return {"env 2's running game has max_moves moves": one.running[2] == trace.case.max_moves == 4,
            "the batch gives it a fifth with no done": two.batches[0]["actions"][0, 2] >= 0 and not two.batches[0]["done"][0, 2],
            "the call is refused for the overflow": two.error == ERR_OVERFLOW and two.calls[0].refused == ERR_OVERFLOW,
            "other envs would have finished games": bool(two.batches[0]["done"][0].any()),
            "nothing changed": (two.counters, two.stored_ids, two.running) == (one.counters, one.stored_ids, one.running) and two.ids == [],
            "the next call works": three.error is None and len(three.ids) > 0}


def reaches_refused(trace):
    one, two = trace.rounds
    good, bad, after = one.calls
    return {"the list's drain falls on the second and the third call": list_plan(trace.case.E, [c.M for c in one.calls])
            == [(True, True), (True, False), (True, False)],
            "the first call files games": good.refused is None and good.n_new > 0,
            "the second is refused for its legal set": bad.refused == ERR_LEGAL,
            "the third is refused with it": after.refused == ERR_LEGAL and max(after.played) > 0,
            "the sync reports it": one.error == ERR_LEGAL,
            "the following sync hands out the first call's games": one.ids == [g[2] for g in good.games] and len(one.ids) > 0,
            "the next call works": two.error is None and len(two.ids) > 0}


BLOCK_EDGES = [Case(f"block_edges_{E}", E, 700, [[call(finish=(E - 1,) + ((BLOCK - 1, BLOCK) if E > BLOCK else ()))],
                                                [call(finish=(E - 1,) + ((BLOCK - 1, BLOCK) if E > BLOCK else ()))]],
                    reaches_block_edges(E), seed=100 + E) for E in (1, 63, 255, 256, 257)]


def _scan_case(E, variant):
    extra = {"plain": dict(finish=(E - 1,) + ((CHUNK - 1, CHUNK) if E > CHUNK else ())),
             "low_zero": dict(stall_at_zero=range(CHUNK)), "high_zero": dict(stall_at_zero=range(CHUNK, E))}[variant]
    name = f"scan_carry_{E}" + ("" if variant == "plain" else "_" + variant)
    return Case(name, E, 8192, [[call(**extra)], [call(**extra)]], reaches_scan(E, variant), seed=200 + E + len(variant),
                small=E <= CHUNK + 1)


SCAN_CARRY = [_scan_case(E, "plain") for E in (1023, 1024, 1025, 2500)] + [_scan_case(2500, "low_zero"),
                                                                           _scan_case(2500, "high_zero")]
WRAP = [Case(f"wrap_inside_a_call_{G}", 2500, G, [[call(stall_rate=0.05, done_rate=0.6)], [call(stall_rate=0.05, done_rate=0.6)]],
             reaches_wrap(G), seed=seed, twin=True, small=False) for G, seed in ((1, 301), (5, 307), (1500, 1800))]
PARTIAL_EVICTION = Case("partial_eviction", 2500, 3000, [[call(stall_rate=0.2, done_rate=0.1)], [call(stall_rate=0.2, done_rate=0.1)]],
                        reaches_partial_eviction, seed=400, next_id=2990, small=False)
LONG_GAME = Case("long_game", 3, 64, [[call(M=65, stall_rate=0.0, done_rate=0.08, quiet=(0, 1))]] * 4, reaches_long_game,
                 seed=661, max_moves=260, td_steps=5, twin=True, small=False)
ACTION_WIDTHS = [Case(f"action_widths_{A}", 70, 256, [[call()], [call()]], reaches_action_widths(A), seed=600 + A, A=A,
                      players=2, legal_form="wide") for A in (1, 64, 65, 121)]
ONE_LEGAL_SET = Case("one_legal_set_for_the_batch", 9, 64, [[call()], [call()]], reaches_one_legal_set, seed=700,
                     legal_form="batch")
OBS_COPIES = [Case(f"obs_{n}" + "".join("_misaligned_" + w for w in mis), 9, 64, [[call()], [call()]], reaches_obs, seed=800 + n,
                   obs_shape=(1, 1, n), misalign=mis)
              for n, mis in ((3, ()), (4, ()), (260, ()), (4, ("obs_after",)), (4, ("obs_next",)))]
BETWEEN_SYNCS = Case("calls_between_syncs", 40, 64, [[call(M=2), call(M=2), call(M=5)]], reaches_between_syncs, seed=900)
REANALYSED = Case("reanalysed_slot", 4, 4, [[call(stall_rate=0.0, done_rate=0.0)],
                                            [call(stall_rate=0.0, done_rate=0.0, stall_at_zero=(2, 3))]], reaches_reanalysed,
                  seed=1000, td_steps=1)
OVERFLOW = Case("overflow", 6, 16, [[call(M=4, stall_rate=0.0, quiet=(2,), unforced=(2,))],
                                    [call(M=1, stall_rate=0.0, done_rate=0.9, quiet=(2,), unforced=(2,))],
                                    [call(stall_at_zero=(2,))]], reaches_overflow, seed=1100, max_moves=4)
REFUSED = Case("refused_call_between_unsynced_calls", 5, 32, [[call(M=2, stall_rate=0.0), call(M=2, stall_rate=0.0, corrupt=(1, 3)),
                                                               call(M=2, stall_rate=0.0)], [call(M=2)]], reaches_refused, seed=1200)

CASES = (BLOCK_EDGES + SCAN_CARRY + WRAP + [PARTIAL_EVICTION, LONG_GAME] + ACTION_WIDTHS + [ONE_LEGAL_SET] + OBS_COPIES
         + [BETWEEN_SYNCS, REANALYSED, OVERFLOW, REFUSED])


# ---- a batch on the device --------------------------------------------------------------------------------------------
def misaligned(tensor):
    """The same values behind a pointer that is 4 bytes past a 16-byte boundary: one float more, sliced [1:]."""
    import torch
    flat = torch.empty(tensor.numel() + 1, dtype=tensor.dtype, device=tensor.device)
    view = flat[1:].view(tensor.shape)
    view.copy_(tensor)
    assert view.data_ptr() % 16 == tensor.element_size() and view.is_contiguous()
    return view


def upload(batch, device, misalign=()):
    """A make_batch dict as device tensors, under the names file_moves reads."""
    import torch
    names = dict(actions="actions", visits="visits", rvs="root_value_sum", legal="legal", num_legal="num_legal",
                 to_play="to_play", last="to_play_last", rewards="rewards", done="done", obs_after="obs_after",
                 obs_next="obs_next")
    keep = {}
    for short, name in names.items():
        a = batch[name]
        keep[short] = None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    for short in misalign:
        keep[short] = misaligned(keep[short])
    return keep


def file_moves(native, keep, n_moves, num_simulations, players, batch_legal=False):
    """A _native.MzReplayFileMoves over the device tensors in `keep` (which must outlive the filing): per-move blocks a
    row of the [M, ...] tensor apart; batch_legal: legal [E, A] / num_legal [E] read with stride 0."""
    mv = native.MzReplayFileMoves()
    mv.n_moves, mv.num_simulations, mv.players = n_moves, num_simulations, players
    for name, key in (("actions", "actions"), ("visits", "visits"), ("root_value_sum", "rvs"), ("legal", "legal"),
                      ("num_legal", "num_legal"), ("to_play", "to_play")):
        t = keep[key]
        if t is None:
            continue
        setattr(mv, name, t.data_ptr())
        stride = 0 if batch_legal and name in ("legal", "num_legal") else t.stride(0) * t.element_size()
        setattr(mv, name + "_stride", stride)
    if keep["last"] is not None:
        mv.to_play_last = keep["last"].data_ptr()
    mv.rewards, mv.done = keep["rewards"].data_ptr(), keep["done"].data_ptr()
    mv.obs_after, mv.obs_next = keep["obs_after"].data_ptr(), keep["obs_next"].data_ptr()
    return mv
