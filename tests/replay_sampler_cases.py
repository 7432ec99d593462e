"""The cases of tests/test_gpu_replay_sampler_forms.py, and the run that plays one of them: against the numpy yardstick
alone (tests/test_replay_sampler_reference.py: every case runs under numpy, is in the form it is named for, and rejects
the defects it is there for) or with a device store beside it, every batch compared bit for bit.

A case is a script over a `Run`: games arrive (`add`), a stream state is loaded (`set_state`), a batch is drawn
(`sample`), priorities are written back (`update`).  Stores are built so that a game's initial priorities are known
without a device: PER_alpha = 1, no rewards and td_steps = max_moves (no bootstrap) make |root value - target| ** alpha
the root value itself, so the float32 rows handed to `add` ARE the priorities priorities_kernel must leave."""
import importlib

import numpy as np

from replay_sampler_reference import ModelStore, sample_batch

# ---- the host's switches (csrc/mzreplay.hip near mzreplay_sample_batch), restated -------------------------------------
LDS_BUDGET = 144 * 1024
MAX_LEAVES = 512
MAX_BATCH = 4096


def lds_games(capacity):
    """game probabilities (4 B) and their running sum (8 B) fit LDS"""
    return 12 * capacity <= LDS_BUDGET


def leaf_count(n):
    """leaves of numpy.sum's float32 tree over n elements: pieces of 8192, halved (down to a multiple of 8) above 128"""
    def tree(m):
        if m <= 128:
            return 1
        half = m // 2 - (m // 2) % 8
        return tree(half) + tree(m - half)
    return sum(tree(min(8192, n - off)) for off in range(0, n, 8192))


def parallel_leaves(n_games):
    return leaf_count(n_games) <= MAX_LEAVES


def lds_rows(max_moves):
    return 8 * max_moves <= LDS_BUDGET


def lds_tails(batch, unroll, max_moves):
    tail = min(unroll, max_moves)
    return 8 * batch * tail + 4 * batch <= LDS_BUDGET


def batch_admitted(batch):
    return 1 <= batch <= MAX_BATCH


# ---- MT19937 words on demand ------------------------------------------------------------------------------------------
def untemper(word):
    """the key word whose tempering is `word`"""
    y = word ^ (word >> 18)
    y ^= (y << 15) & 0xEFC60000
    t = y
    for _ in range(5):
        t = y ^ ((t << 7) & 0x9D2C5680)
    y = t & 0xFFFFFFFF
    t = y
    for _ in range(3):
        t = y ^ (t >> 11)
    return t & 0xFFFFFFFF


def key_for_doubles(doubles, filler_seed=77):
    """A key block which, read from position 0, gives exactly these legacy doubles (multiples of 2 ** -53 below 1)."""
    key = np.random.RandomState(filler_seed).get_state()[1].copy()
    assert 2 * len(doubles) <= 624
    for i, u in enumerate(doubles):
        k = int(u * 2 ** 53)
        assert 0 <= k < 2 ** 53 and k / 2 ** 53 == u
        key[2 * i] = untemper((k >> 26) << 5)
        key[2 * i + 1] = untemper((k & (2 ** 26 - 1)) << 6)
    return key


STREAM_KEY = np.random.RandomState(20240601).get_state()[1].copy()   # the fixed block of the stream-position cases
EPS = 2.0 ** -53


# ---- one run of a case --------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, script, capacity, max_moves, actions, unroll, seed=3, host=True):
        self.name, self.script = name, script
        self.capacity, self.max_moves, self.actions, self.unroll, self.seed, self.host = \
            capacity, max_moves, actions, unroll, seed, host

    def config(self):
        config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
        config.action_space = list(range(self.actions))
        config.observation_shape, config.stacked_observations = (1, 1, 2), 0
        config.max_moves, config.replay_buffer_size, config.batch_size = self.max_moves, self.capacity, 1
        config.PER, config.PER_alpha, config.num_unroll_steps, config.td_steps = True, 1, self.unroll, self.max_moves
        config.seed = self.seed
        return config


class Run:
    """Plays a case.  Without `mods` only the yardstick runs (and every batch is recorded with its inputs); with
    mods = (replay_buffer module, self_play module) a device-sampled store -- and, where the case allows, a host-sampled
    one on the same games -- runs beside it and every step is compared."""

    def __init__(self, case, mods=None):
        self.case, self.model = case, ModelStore(case.capacity)
        self.rs = np.random.RandomState(case.seed)             # ReplayBuffer seeds the sampler with config.seed
        self.records, self.last = [], None
        self.dev = self.host = None
        self.fill = np.random.RandomState(case.seed + 1)
        if mods is not None:
            rb_mod, self.sp = mods
            self.config = case.config()
            start = {"num_played_games": 0, "num_played_steps": 0}
            self.dev = rb_mod.ReplayBuffer(start, {}, self.config, device_sampling=True)
            if case.host:
                self.host = rb_mod.ReplayBuffer(start, {}, self.config)

    def close(self):
        for rb in (self.dev, self.host):
            if rb is not None:
                rb.close()

    # -- games arrive
    def _packed(self, rows):
        n, L, A = len(rows), self.case.max_moves, self.case.actions
        length = np.array([len(r) for r in rows], dtype=np.int32)
        root_values = np.zeros((n, L), dtype=np.float64)
        for g, row in enumerate(rows):
            root_values[g, : len(row)] = row
        obs = np.zeros((n, L + 1, 1, 1, 2), dtype=np.float32)
        obs[:, :, 0, 0, 0] = np.arange(L + 1, dtype=np.float32) % 97
        obs[:, :, 0, 0, 1] = (self.model.first_id + len(self.model) + np.arange(n, dtype=np.float32))[:, None] % 89
        return self.sp.PackedGames(env_index=np.arange(n), length=length, observations=obs,
                                   actions=self.fill.randint(0, A, size=(n, L + 1)).astype(np.int32),
                                   rewards=np.zeros((n, L + 1)), to_play=np.zeros((n, L + 1), dtype=np.int32),
                                   child_visits=np.full((n, L, A), 1.0 / A), root_values=root_values)

    def add(self, rows, spot_check=64):
        rows = [np.array(r, dtype=np.float32) for r in rows]
        if self.dev is not None:
            self.config.PER = True         # (sample() sets it per batch; the host store keeps priorities only under PER)
            packed = self._packed(rows)
            first = self.dev.num_played_games
            self.dev.save_games(packed)
            if self.host is not None:      # the same priorities_kernel, its rows copied back: all of them are looked at
                self.host.save_games(packed)
                for g, row in enumerate(rows):
                    entry = self.host.buffer.get(first + g)
                    if entry is not None:
                        assert np.array_equal(entry["priorities"].view(np.uint32), row.view(np.uint32)), first + g
                        assert entry["game_priority"] == np.max(row)
            kept = [g for g in range(len(rows)) if first + g in self.dev.buffer]
            picks = kept if len(kept) <= spot_check else \
                sorted(set(self.fill.choice(kept, spot_check - 2).tolist()) | {kept[0], kept[-1]})
            for g in picks:                # what adopt_games_kernel left in the sampler's arrays
                got, got_game = self.dev.download_priorities(first + g)
                assert np.array_equal(got.view(np.uint32), rows[g].view(np.uint32)), first + g
                assert got_game == np.max(rows[g])
        self.model.add(rows)
        if self.dev is not None:
            assert len(self.dev.buffer) == len(self.model) and self.dev.total_samples == self.model.total_samples
            assert self.dev.num_played_games - len(self.dev.buffer) == self.model.first_id

    # -- the stream
    def set_state(self, key, pos):
        state = ("MT19937", np.array(key, dtype=np.uint32), int(pos), 0, 0.0)
        self.rs.set_state(state)
        if self.dev is not None:
            self.dev.set_sampler_state(state)

    # -- one batch
    def sample(self, batch, per, label, **forms):
        """forms: the switch sides this batch is named for, e.g. lds_games=False -- asserted against the predicates."""
        case, model = self.case, self.model
        here = dict(lds_games=lds_games(case.capacity), parallel_leaves=parallel_leaves(len(model)),
                    lds_rows=lds_rows(case.max_moves), lds_tails=lds_tails(batch, case.unroll, case.max_moves),
                    wrapped=model.first_id % case.capacity != 0)
        for name, side in forms.items():
            assert here[name] == side, (case.name, label, name, here[name])
        before = self.rs.get_state()
        game_priority, lengths, priorities, total = model.snapshot()
        want = sample_batch(self.rs, game_priority, lengths, priorities, batch, case.unroll, case.actions, per, total)
        self.last = dict(label=label, batch=batch, per=per, before=before, inputs=(game_priority, lengths, priorities, total),
                         want=want, first_id=model.first_id, forms=here)
        self.records.append(self.last)
        if self.dev is not None:
            self._compare(want, batch, per, before, lengths, label)
        return want

    def _compare(self, want, batch, per, before, lengths, label):
        import torch
        from test_gpu_replay_sampler import assert_same_batch
        self.config.batch_size, self.config.PER = batch, per
        got = self.dev.get_batch()
        index, (obs, act, val, rew, pol, weight, scale) = got
        ids, positions = index.game_ids.cpu().numpy(), index.positions.cpu().numpy()
        assert ids.dtype == np.int64 and positions.dtype == np.int32
        assert np.array_equal(ids, self.model.first_id + want["game_index"]), label
        assert np.array_equal(index.slots.cpu().numpy(), ids % self.case.capacity), label
        assert np.array_equal(positions, want["position"]), label
        past = want["position"][:, None] + np.arange(self.case.unroll + 1)[None, :] > lengths[want["game_index"]][:, None]
        assert np.array_equal(act.cpu().numpy()[past], want["absorbing"][past]), label
        if per:
            assert weight.dtype == torch.float32
            assert np.array_equal(weight.cpu().numpy().view(np.uint32), want["weight"].view(np.uint32)), label
        else:
            assert weight is None
        state = self.dev.sampler_state()
        assert state[2] == want["state"][2] and np.array_equal(state[1], want["state"][1]), label
        self.last["device_index"] = index
        if self.host is not None:
            self.host.rng.set_state(before)
            assert_same_batch(self.host.get_batch(), got, per)
            after = self.host.rng.get_state()
            assert after[2] == want["state"][2] and np.array_equal(after[1], want["state"][1]), label

    def refused(self, batch):
        """a batch size the sampler does not take: refused by name, the stream where it was"""
        assert not batch_admitted(batch)
        if self.dev is None:
            return
        import pytest
        before = self.dev.sampler_state()
        self.config.batch_size = batch
        with pytest.raises(RuntimeError, match=r"batch must be 1\.\.4096"):
            self.dev.get_batch()
        after = self.dev.sampler_state()
        assert after[2] == before[2] == self.rs.get_state()[2] and np.array_equal(after[1], before[1])
        assert np.array_equal(after[1], self.rs.get_state()[1])

    # -- priorities come back
    def update(self, seed):
        """update_priorities on the last batch with fresh values; the touched games are read back and compared."""
        last = self.last
        batch, U1 = last["batch"], self.case.unroll + 1
        rs = np.random.RandomState(seed)
        fresh = rs.choice(np.array([0, 1e-12, 1e3, 0.5, 2.0], dtype=np.float32), size=(batch, U1)).astype(np.float32)
        fresh[rs.random_sample(fresh.shape) < 0.5] += np.float32(rs.random_sample())
        ids = last["first_id"] + last["want"]["game_index"]
        touched = self.model.update(ids, last["want"]["position"], fresh)
        if self.dev is not None:
            import torch
            self.dev.update_priorities(torch.from_numpy(fresh).cuda(), last["device_index"])
            for gid in sorted(set(touched)):
                got, got_game = self.dev.download_priorities(gid)
                g = gid - self.model.first_id
                assert np.array_equal(got.view(np.uint32), self.model.priorities[g].view(np.uint32)), gid
                assert got_game == self.model.game_priority[g], gid
            if self.host is not None:
                self.host.update_priorities(fresh, [[int(i), int(p)] for i, p in zip(ids, last["want"]["position"])])
        return touched


# ---- priorities ---------------------------------------------------------------------------------------------------------
def mixed(rs, n, zeros=0.3):
    """float32 over fifteen decades, about 30 % zeros: every pairwise addition rounds"""
    a = (10.0 ** rs.uniform(-12, 3, size=n)).astype(np.float32)
    a[rs.random_sample(n) < zeros] = 0
    return a


def pairwise_tree(a):
    """numpy's pairwise float32 sum as ONE tree over all of `a` (numpy.sum itself works in pieces of 8192)"""
    if len(a) <= 128:
        return np.sum(a)
    half = len(a) // 2 - (len(a) // 2) % 8
    return pairwise_tree(a[:half]) + pairwise_tree(a[half:])


def short_games(seed, n, telling=()):
    """n games of 1-2 plies with mixed priorities; the first two are not all zero.  The seed moves on until, at every
    game count in `telling`, numpy.sum of the game priorities is neither their left-to-right sum nor the sum of one
    pairwise tree over all of them: a sampler that adds them up in another order then gets other probabilities."""
    while True:
        rs = np.random.RandomState(seed)
        lengths = rs.randint(1, 3, size=n)
        flat = mixed(rs, int(lengths.sum()))
        rows = np.split(flat, np.cumsum(lengths)[:-1])
        for row in rows[:2]:
            row[0] = row[0] if row[0] > 0 else np.float32(0.75)
        top = np.array([np.max(row) for row in rows], dtype=np.float32)
        if all(np.sum(top[:m]) != np.add.accumulate(top[:m])[-1] and np.sum(top[:m]) != pairwise_tree(top[:m])
               for m in telling):
            return rows
        seed += 1000


# ---- game forms -----------------------------------------------------------------------------------------------------------
BATCH = 61


def both(run, label, **forms):
    run.sample(BATCH, True, label + " per", **forms)
    run.sample(BATCH, False, label + " uniform", **forms)


def game_forms_script(capacity):
    def script(run):
        side = dict(lds_games=capacity <= 12288, parallel_leaves=True)
        rows = short_games(capacity, capacity + 100, telling=(capacity,))
        at = 0
        for n in (1, 2, capacity - 1, capacity):
            run.add(rows[at:n])
            at = n
            both(run, f"n={n}", wrapped=False, **side)
        run.add(rows[at:])                                     # 100 more than the ring holds: ring order != slot order
        both(run, "wrapped", wrapped=True, **side)
        assert run.model.first_id == 100 and len(run.model) == capacity
        run.update(seed=capacity + 1)
        both(run, "updated", wrapped=True, **side)
    return script


LEAF_EDGES = (65032, 65033, 65040, 65536, 65537, 70001)       # 512 | 513 | 512 | 512 | 513 | 551 leaves


def leaf_forms_script(run):
    rows = short_games(70001, LEAF_EDGES[-1], telling=(65033, 65537))
    at = 0
    for n in LEAF_EDGES:
        run.add(rows[at:n])
        at = n
        both(run, f"n={n}", lds_games=False, parallel_leaves=n in (65032, 65040, 65536), wrapped=False)
    run.update(seed=5)
    both(run, "updated", lds_games=False, parallel_leaves=False)


# ---- position forms -------------------------------------------------------------------------------------------------------
def long_row(rs, n, unroll=5):
    """every addition rounds, and the last `unroll` entries hold about half of the mass"""
    while True:
        row = rs.uniform(0.5, 1.5, size=n).astype(np.float32)
        row[-unroll:] = np.float32(n / unroll) * rs.uniform(0.75, 1.25, size=unroll).astype(np.float32)
        if np.float32(sum(row)) != np.sum(row):                # Python's sum is not numpy's on this row
            return row


def position_forms_script(L):
    def script(run):
        rs = np.random.RandomState(L)
        rows = [long_row(rs, L), long_row(rs, L - 1), np.array([L / 10], dtype=np.float32)]
        for row in rows[:2]:
            assert np.float32(sum(row)) != np.sum(row)
        run.add(rows)
        side = dict(lds_rows=L <= 18432, lds_games=True, lds_tails=True)
        for i in range(4):
            run.sample(1, True, f"batch 1 #{i}", **side)
        for i in range(3):
            run.sample(5, True, f"batch 5 #{i}", **side)
        run.sample(5, False, "batch 5 uniform", **side)
        run.sample(5, True, "batch 5 before the update", **side)
        run.update(seed=L)
        run.sample(5, True, "batch 5 updated", **side)
        run.sample(1, True, "batch 1 updated", **side)
        # the cases are there for what they name: the table's last entries and its body, and the one-ply game
        lengths = np.array([L, L - 1, 1])
        seen = [(int(lengths[g]), int(p)) for r in run.records if r["per"]
                for g, p in zip(r["want"]["game_index"], r["want"]["position"])]
        assert any(n > 1 and p >= n - run.case.unroll for n, p in seen), "no position in the table's tail"
        assert any(n > 1 and p < n - run.case.unroll for n, p in seen), "no position before the tail"
        assert any(n == 1 for n, _ in seen) and any(n == L for n, _ in seen) and any(n == L - 1 for n, _ in seen)
    return script


# ---- walk forms, and one store at several batch sizes ---------------------------------------------------------------------
def small_store(run, seed):
    rs = np.random.RandomState(seed)
    lengths = [1, 9, 4, 5, 6, 2, 8]
    rows = [mixed(rs, n, zeros=0.2) for n in lengths]
    for row in rows:
        row[rs.randint(len(row))] = np.float32(rs.uniform(0.5, 2))   # no all-zero game
    run.add(rows)


def walk_forms_u5_script(run):
    small_store(run, 51)
    run.sample(3351, True, "batch 3351", lds_tails=True, lds_rows=True, lds_games=True)
    run.sample(3352, True, "batch 3352", lds_tails=False)
    run.sample(4096, True, "batch 4096", lds_tails=False)
    run.sample(4096, False, "batch 4096 uniform")
    run.refused(4097)
    run.sample(3351, True, "batch 3351 again", lds_tails=True)


def walk_forms_u4_script(run):
    small_store(run, 41)
    assert 4096 * (8 * 4 + 4) == LDS_BUDGET                 # exactly the budget
    run.sample(4096, True, "batch 4096", lds_tails=True)
    run.refused(4097)


def several_batches_script(run):
    small_store(run, 7)
    for i, batch in enumerate((1, 129, 4096, 1)):            # the per-batch scratch grows twice, then is reused
        run.sample(batch, True, f"#{i} batch {batch}")
    run.update(seed=8)
    run.sample(129, True, "updated batch 129")


# ---- every stream position ------------------------------------------------------------------------------------------------
def stream_script(per, rows_of):
    def script(run):
        run.add(rows_of(np.random.RandomState(run.case.actions)))
        for pos in range(625):
            run.set_state(STREAM_KEY, pos)
            run.sample(5, per, f"pos {pos}")
    return script


def short_rows(rs):
    return [mixed(rs, n, zeros=0.0) for n in (1, 2, 3, 4, 2, 1)]        # all shorter than the unroll of 5


def one_ply_rows(rs):
    return [mixed(rs, 1, zeros=0.0) for _ in range(6)]


# ---- chosen draws -----------------------------------------------------------------------------------------------------------
def chosen_script(rows, game_draws, position_draws, want_games, want_positions, scale=1.0, check=None):
    """Batch B = len(game_draws) with one action: the stream is B game doubles, then B position doubles."""
    def script(run):
        run.add([np.array(r, dtype=np.float32) * np.float32(scale) for r in rows])
        if check is not None:
            check(run)
        run.set_state(key_for_doubles(list(game_draws) + list(position_draws)), 0)
        want = run.sample(len(game_draws), True, "chosen")
        assert want["game_index"].tolist() == list(want_games), want["game_index"]
        assert want["position"].tolist() == list(want_positions), want["position"]
        assert want["state"][2] == 4 * len(game_draws)
    return script


EQUAL_GAMES = dict(rows=[(1, 0, 0, 1, 2)] * 4,               # game table .25 .5 .75 1; position table .25 .25 .25 .5 1
                   game_draws=(0.0, 0.25, 0.5, 0.75, 1 - EPS, 0.25 - EPS), want_games=(0, 1, 2, 3, 3, 0),
                   position_draws=(0.0, 0.25, 0.5, 1 - EPS, 0.25 - EPS, 0.5 - EPS), want_positions=(0, 3, 4, 4, 0, 3))
ZERO_GAMES = dict(rows=[(0,), (0, 0, 1, 0), (0, 0), (0,), (1,), (0, 1, 2, 1, 0), (0,)],   # game table 0 .25 .25 .25 .5 1 1
                  game_draws=(0.0, 0.25, 0.5, 1 - EPS, 0.25 - EPS, 0.5 - EPS), want_games=(1, 4, 5, 5, 1, 4),
                  position_draws=(0.0, 0.5, 0.25, 1 - EPS, 1 - EPS, 0.0), want_positions=(2, 0, 2, 3, 2, 0))
SUBNORMAL = 2.0 ** -140


def third_check(run):
    """three equal games: float32(1/3) three times is not 1 in fp64, so choice()'s division by the last entry matters"""
    game_priority, _, priorities, _ = run.model.snapshot()
    for p in (game_priority, priorities[1]):
        last = np.cumsum((p / np.sum(p)).astype(np.float64))[-1]
        assert last != 1.0 and float(p[0] / np.sum(p)) / last < float(p[0] / np.sum(p))


def third_draw():
    q = float(np.float32(1) / np.float32(3))
    u = np.ceil(q / (q + q + q) * 2 ** 53) / 2 ** 53         # at or past the renormalised first entry, below the raw one
    assert q / (q + q + q) <= u < q
    return u


THIRDS = dict(rows=[(1, 1, 1)] * 3, game_draws=(third_draw(),), want_games=(1,), position_draws=(third_draw(),),
              want_positions=(1,), check=third_check)


def build_cases():
    cases = [Case("games G=12288", game_forms_script(12288), 12288, 2, 3, 5),
             Case("games G=12289", game_forms_script(12289), 12289, 2, 3, 5),
             Case("leaves n=65032..70001", leaf_forms_script, 70001, 2, 3, 5)]
    cases += [Case(f"positions L={L}", position_forms_script(L), 3, L, 2, 5, seed=L) for L in (18432, 18433, 27000)]
    cases += [Case("walk U=5", walk_forms_u5_script, 8, 9, 3, 5), Case("walk U=4", walk_forms_u4_script, 8, 9, 3, 4),
              Case("several batches", several_batches_script, 8, 9, 3, 5)]
    for A in (1, 2, 3, 121):
        for per in (True, False):
            cases.append(Case(f"stream A={A} {'per' if per else 'uniform'}", stream_script(per, short_rows), 6, 4, A, 5,
                              host=False))
    for per in (True, False):
        cases.append(Case(f"stream U=121 {'per' if per else 'uniform'}", stream_script(per, one_ply_rows), 6, 1, 3, 121,
                          host=False))
    cases += [Case("chosen equal games", chosen_script(**EQUAL_GAMES), 4, 5, 1, 5),
              Case("chosen zero games", chosen_script(**ZERO_GAMES), 7, 5, 1, 5),
              Case("chosen equal games subnormal", chosen_script(scale=SUBNORMAL, **EQUAL_GAMES), 4, 5, 1, 5),
              Case("chosen zero games subnormal", chosen_script(scale=SUBNORMAL, **ZERO_GAMES), 7, 5, 1, 5),
              Case("chosen last != 1", chosen_script(**THIRDS), 3, 3, 1, 5)]
    return cases


CASES = build_cases()
CASE_NAMES = [case.name for case in CASES]


def case_named(name):
    return CASES[CASE_NAMES.index(name)]
