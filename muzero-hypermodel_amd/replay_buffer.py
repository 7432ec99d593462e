"""ReplayBuffer with the reference's interface (replay_buffer.py:11-295) over the device-resident replay
store (include/mzreplay.h): finished games live on the GPU as packed arrays, initial priorities and the
training targets of a batch are computed there, and `get_batch` returns device tensors.

What stays on the host, as in the reference: which games / positions are sampled and the random actions of
absorbing states, drawn in the reference's order from a numpy-compatible legacy stream seeded with
config.seed (the reference seeds numpy's global stream in the buffer's own process, replay_buffer.py:31).
Sampling reads the priorities, which are mirrored on the host (a few floats per game).

With `device_sampling=True` the sampling moves to the device as well (include/mzreplay.h mzreplay_sample_batch,
csrc/replay_sampler.h): priorities, game priorities and a numpy stream of its own live in the store, `get_batch` queues
the sampler and the target kernels and returns without waiting, and `update_priorities` takes the trainer's device
tensor -- draw for draw what the host path returns.

With `DeviceSelfPlay.file_to(replay_buffer)` the producer side is on the device too (include/mzreplay.h mzreplay_filer_*,
csrc/replay_filer.h): the actor's finished games go from the search engine's and the environment kernels' device rings
straight into the store's slots, and only their lengths (4 bytes per game) and the counters come back, once per move
batch (`sync_filing`).  Such games have no host copy: `download_games` reads them back when someone asks.  Several actors
(the groups of a `PipelinedDeviceSelfPlay`, or separate `DeviceSelfPlay`s that ask for it with `shared=True`) may file into one store, each through a
`DeviceFiler` and a stream of its own: the store numbers games in the order the filings are queued, whatever the streams do.

Reanalyse refreshes the stored games' value targets with the current network, one game per call
(`Reanalyse.reanalyse_game`, the reference's loop body) or N games per pass queued on one stream
(`Reanalyse.reanalyse_games`; include/mzreplay.h mzreplay_reanalyse_*, csrc/reanalyse_plan.h): the games are drawn on the
device from a stream of the pass's own, every position of every drawn game is evaluated as one batch and the values go
back into the store -- for fully-connected networks in one HIP launch with no host round trip at all.

Not carried over: Ray (`.remote`), `get_buffer()`'s live GameHistory objects are only kept when games
arrive as GameHistory (save_game), and `update_game_history` (the values live in the store, not in a GameHistory).
"""
import ctypes
import itertools

import numpy
import torch

from . import _native
from ._native import c_f32_p, c_f64_p, c_i32_p, ptr


class MzReplayConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("capacity", "max_moves", "num_actions", "obs_channels", "obs_height",
                                              "obs_width", "stacked_observations", "td_steps", "num_unroll_steps",
                                              "device")] + \
               [("per_alpha", ctypes.c_double), ("discount_powers", ctypes.c_void_p)]


class DeviceIndexBatch:
    """index_batch of a device-sampled batch: game_ids i64[B], positions i32[B] (and the slots the targets were read
    from) as CUDA tensors.  `tolist()` gives the reference's list of [game_id, game_pos] pairs, waiting for the device."""

    def __init__(self, game_ids, slots, positions):
        self.game_ids, self.slots, self.positions = game_ids, slots, positions

    def __len__(self):
        return int(self.game_ids.shape[0])

    def tolist(self):
        return [list(pair) for pair in zip(self.game_ids.tolist(), self.positions.tolist())]


class ReanalysePlan:
    """The plan of a batched Reanalyse pass (csrc/reanalyse_plan.h), as CUDA tensors: game_ids i64[n], slots i32[n],
    row_start i32[n + 1] (row_start[n] = the rows R of the pass).  Draws whose game is drawn again later in the pass have
    no rows.  The tensors belong to the buffer and are rewritten by its next plan of the same size."""

    def __init__(self, n_games, game_ids, slots, row_start, max_rows):
        self.n_games, self.game_ids, self.slots, self.row_start, self.max_rows = n_games, game_ids, slots, row_start, max_rows

    def rows(self):
        """R, read back from the device (4 bytes; waits for it)."""
        return int(self.row_start[self.n_games].item())


class _DeviceEntry(dict):
    """A buffer entry whose priorities live in the store: "priorities" / "game_priority" are downloaded when asked for,
    assigning "priorities" uploads them (the game priority follows as their maximum)."""

    def __init__(self, owner, game_id, **fields):
        super().__init__(**fields)
        self._owner, self._game_id = owner, game_id

    def __getitem__(self, key):
        if key == "priorities":
            return self._owner.download_priorities(self._game_id)[0]
        if key == "game_priority":
            return self._owner.download_priorities(self._game_id)[1]
        return super().__getitem__(key)

    def __setitem__(self, key, value):
        if key == "priorities":
            self._owner.load_priorities(self._game_id, value)
        elif key == "game_priority":
            raise KeyError("the game priority of a device-sampled buffer is the maximum of the priorities it holds")
        else:
            super().__setitem__(key, value)


class DeviceFiler:
    """One actor's filer on a ReplayBuffer's store (ReplayBuffer.attach_filer): the running rows of its `num_envs` envs,
    its list of filed games and its error word.  `begin` / `file` / `lengths` address it; `take_filed` hands its owner the
    games the syncs have fetched for it (ReplayBuffer.sync_filing syncs every filer of the store at once)."""

    def __init__(self, buffer, handle, num_envs, outcomes=False):
        self.buffer, self.handle, self.num_envs = buffer, handle, int(num_envs)
        self.outcomes = bool(outcomes)                    # the filer reports every finished game's outcome (attach_filer)
        self.pending = False                              # a move batch was filed and not synced yet
        self.refused = False                              # its last sync failed: the next one asks it again
        self._filed = []                                  # (env_index, length, game_id) per sync, not yet taken
        self._filed_outcomes = []                         # GAME_OUTCOME_DTYPE records per sync, parallel to _filed
        self._handed = []                                 # self_play.GameOutcomes of the games take_filed handed out

    def begin(self, first_observations, first_to_play=None):
        self.buffer.filer_begin(first_observations, first_to_play, filer=self)

    def file(self, moves):
        self.buffer.filer_file(moves, filer=self)

    def lengths(self):
        return self.buffer.filer_lengths(filer=self)

    def take_filed(self):
        """This filer's games since it last took them: (env_index, length, game_id) host arrays, ids ascending; syncs the
        store's filers first when this one has a filing pending."""
        if self.pending:
            self.buffer._sync_filers()
        taken, self._filed = self._filed, []
        if self.outcomes:
            from .self_play import GameOutcomes
            self._handed += [GameOutcomes.from_records(*filed, records) for filed, records in zip(taken, self._filed_outcomes)]
            self._filed_outcomes = []
        if len(taken) == 1:
            return taken[0]
        dtypes = (numpy.int32, numpy.int32, numpy.int64)
        return tuple(numpy.concatenate([t[i] for t in taken]) if taken else numpy.zeros(0, dtype=dtypes[i]) for i in range(3))

    def take_outcomes(self):
        """The outcomes of the games take_filed has handed out since the last take_outcomes, in that order: a
        self_play.GameOutcomes.  The filer computed them where it finished the games (40 bytes per game came back with the
        sync); a filer attached without outcomes=True has none and raises."""
        if not self.outcomes:
            raise RuntimeError("this filer reports no outcomes: turn them on when the actor starts filing, "
                               "file_to(replay_buffer, outcomes=True) (ReplayBuffer.attach_filer(num_envs, outcomes=True))")
        from .self_play import GameOutcomes
        handed, self._handed = self._handed, []
        return GameOutcomes.concatenate(handed)


class ReplayBuffer:
    def __init__(self, initial_checkpoint, initial_buffer, config, device=None, device_sampling=False):
        """device_sampling=True: get_batch / update_priorities run on the device (see the module docstring).  Batch
        sampling then has a stream of its own, seeded with config.seed; sample_game / sample_position (Reanalyse and
        other host callers) keep drawing from the host generator -- as in the reference, where Reanalyse is another
        process with its own numpy stream."""
        if not torch.cuda.is_available():
            raise RuntimeError("the device replay store needs a HIP device (there is no CPU fallback)")
        self.config = config
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _native.load()
        self.num_played_games = initial_checkpoint["num_played_games"]
        self.num_played_steps = initial_checkpoint["num_played_steps"]
        self.total_samples = 0
        self.A = len(config.action_space)
        self.C, self.H, self.W = (int(v) for v in config.observation_shape)
        self.L = int(config.max_moves)
        self.capacity = int(config.replay_buffer_size)
        self.U1 = int(config.num_unroll_steps) + 1
        # discount ** i as Python computes it (replay_buffer.py:240, 253)
        powers = numpy.array([config.discount ** i for i in range(config.td_steps + 1)], dtype=numpy.float64)
        cfg = MzReplayConfig(self.capacity, self.L, self.A, self.C, self.H, self.W, int(config.stacked_observations),
                             int(config.td_steps), int(config.num_unroll_steps), self.device.index,
                             float(config.PER_alpha), powers.ctypes.data)
        handle = ctypes.c_void_p()
        if self._lib.mzreplay_create(ctypes.byref(cfg), ctypes.byref(handle)) != 0:
            raise RuntimeError(self._lib.mzreplay_last_error(None).decode())
        self._h = handle
        self.rng = _native.HostRng(config.seed)           # numpy.random.seed(self.config.seed)
        self.device_sampling = bool(device_sampling)
        if self.device_sampling:
            if list(config.action_space) != list(range(self.A)):
                raise NotImplementedError("device sampling draws absorbing actions as indices: action_space must be range(A)")
            self._check(self._lib.mzreplay_sampler_enable(self._h, int(config.seed) & 0xFFFFFFFF, int(self.num_played_games)))
        self.buffer = {}                                  # game_id -> dict(length, priorities, game_priority[, history])
        self._filers = []                                 # DeviceFiler per filing actor (attach_filer)
        self._unbooked = []                               # (filer, games) synced while another filer's sync failed
        self._reanalyse_plans = {}                        # n_games -> ReanalysePlan (the pass's device arrays, kept)
        # the batched Reanalyse pass draws from a stream of its own, seeded like the reference's Reanalyse worker
        # (numpy.random.seed(config.seed), replay_buffer.py:309); the buffer's and the batch sampler's never move for it
        self._check(self._lib.mzreplay_reanalyse_enable(self._h, int(config.seed) & 0xFFFFFFFF))
        for game_history in (initial_buffer or {}).values():
            self.save_game(game_history)

    # ---- plumbing -----------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.mzreplay_last_error(self._h).decode())

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        for filer in getattr(self, "_filers", []):
            self._lib.mzreplay_filer_destroy(filer.handle)
        self._filers = []
        if getattr(self, "_h", None):
            self._lib.mzreplay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self):
        return int(self._lib.mzreplay_device_bytes(self._h))

    def _slot(self, game_id):
        return game_id % self.capacity

    # ---- save_game (replay_buffer.py:33-65) ----------------------------------------------------------
    def save_game(self, game_history, shared_storage=None):
        n = len(game_history.root_values)
        obs = numpy.zeros((1, self.L + 1, self.C, self.H, self.W), dtype=numpy.float32)
        obs[0, : n + 1] = numpy.asarray(game_history.observation_history, dtype=numpy.float32).reshape(n + 1, self.C, self.H, self.W)
        act = numpy.zeros((1, self.L + 1), dtype=numpy.int32)
        act[0, : n + 1] = game_history.action_history
        rew = numpy.zeros((1, self.L + 1), dtype=numpy.float64)
        rew[0, : n + 1] = game_history.reward_history
        tp = numpy.zeros((1, self.L + 1), dtype=numpy.int32)
        tp[0, : n + 1] = game_history.to_play_history
        cv = numpy.zeros((1, self.L, self.A), dtype=numpy.float64)
        cv[0, :n] = game_history.child_visits
        rv = numpy.zeros((1, self.L), dtype=numpy.float64)
        rv[0, :n] = game_history.root_values
        self._add(numpy.array([n], dtype=numpy.int32), obs, act, rew, tp, cv, rv, [game_history], shared_storage)

    def save_games(self, packed, shared_storage=None):
        """A batch of finished games as arrays (self_play.PackedGames): no per-game Python objects."""
        n_games, width = len(packed), packed.actions.shape[1] - 1

        def padded(a, tail, dtype):
            out = numpy.zeros((n_games, tail) + a.shape[2:], dtype=dtype)
            out[:, : a.shape[1]] = a
            return out
        self._add(numpy.ascontiguousarray(packed.length, dtype=numpy.int32),
                  padded(packed.observations.reshape(n_games, width + 1, self.C, self.H, self.W), self.L + 1, numpy.float32),
                  padded(packed.actions, self.L + 1, numpy.int32), padded(packed.rewards, self.L + 1, numpy.float64),
                  padded(packed.to_play, self.L + 1, numpy.int32), padded(packed.child_visits, self.L, numpy.float64),
                  padded(packed.root_values, self.L, numpy.float64), [None] * n_games, shared_storage)

    def _add(self, lengths, obs, act, rew, tp, cv, rv, histories, shared_storage):
        self._sync_if_pending()
        n_games = len(lengths)
        ids = numpy.arange(self.num_played_games, self.num_played_games + n_games)
        slots = numpy.ascontiguousarray(ids % self.capacity, dtype=numpy.int32)
        pri = numpy.zeros((n_games, self.L), dtype=numpy.float32)
        game_pri = numpy.zeros(n_games, dtype=numpy.float32)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_add_games(
                self._h, n_games, ptr(slots, c_i32_p), ptr(lengths, c_i32_p), ptr(obs, c_f32_p), ptr(act, c_i32_p),
                ptr(rew, c_f64_p), ptr(tp, c_i32_p), ptr(cv, c_f64_p), ptr(rv, c_f64_p), ptr(pri, c_f32_p),
                ptr(game_pri, c_f32_p), self._stream()))
        for g in range(n_games):
            n = int(lengths[g])
            entry = dict(length=n, history=histories[g])
            if self.device_sampling:
                entry = _DeviceEntry(self, self.num_played_games, length=n, history=histories[g])
                given = getattr(histories[g], "priorities", None) if histories[g] is not None else None
                if self.config.PER and given is not None:
                    self.buffer[self.num_played_games] = entry
                    self.load_priorities(self.num_played_games, given)
            elif self.config.PER:
                given = getattr(histories[g], "priorities", None) if histories[g] is not None else None
                entry["priorities"] = numpy.copy(given) if given is not None else pri[g, :n].copy()
                entry["game_priority"] = numpy.max(entry["priorities"]) if given is not None else game_pri[g]
                if histories[g] is not None:
                    histories[g].priorities, histories[g].game_priority = entry["priorities"], entry["game_priority"]
            self.buffer[self.num_played_games] = entry
            self.num_played_games += 1
            self.num_played_steps += n
            self.total_samples += n
            if self.config.replay_buffer_size < len(self.buffer):
                del_id = self.num_played_games - len(self.buffer)
                self.total_samples -= self.buffer[del_id]["length"]
                del self.buffer[del_id]
        if self._filers:
            self._push_counters()
        if shared_storage:
            shared_storage.set_info("num_played_games", self.num_played_games)
            shared_storage.set_info("num_played_steps", self.num_played_steps)

    def get_buffer(self):
        """game id -> GameHistory.  Games that were filed on the device have no host copy: they are read back here."""
        self._sync_if_pending()
        missing = [gid for gid, e in self.buffer.items() if dict.get(e, "history") is None]
        packed = self.download_games(missing) if missing else None
        fetched = {gid: packed.history(i) for i, gid in enumerate(missing)}
        return {gid: fetched[gid] if gid in fetched else e["history"] for gid, e in self.buffer.items()}

    # ---- games filed on the device (include/mzreplay.h mzreplay_filer_*) ---------------------------------
    def attach_filer(self, num_envs, outcomes=False):
        """A device filer on this store for an actor of `num_envs` envs (DeviceSelfPlay.file_to calls this): a DeviceFiler.
        Several actors may file into one store, each through a filer and a stream of its own: the store numbers games in
        the order of the filer_file calls made on it, whatever stream each runs on (include/mzreplay.h).
        outcomes=True: the filer also reports every finished game's outcome (mzreplay_filer_enable_outcomes; the owner
        reads them with DeviceFiler.take_outcomes)."""
        self._sync_if_pending()                              # (the counters pushed below are the host's)
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_filer_create(self._h, int(num_envs), ctypes.byref(handle)))
            if outcomes:
                self._check(self._lib.mzreplay_filer_enable_outcomes(handle, 1))
        filer = DeviceFiler(self, handle, num_envs, outcomes=outcomes)
        self._filers.append(filer)
        self._push_counters()
        return filer

    @property
    def filers(self):
        """The DeviceFilers attached so far, in the order they were attached."""
        return tuple(self._filers)

    def _the_filer(self, filer):
        """The filer a call addresses: the one given, or the store's only one."""
        if filer is not None:
            return filer
        if len(self._filers) != 1:
            raise RuntimeError("no actor files into this buffer (DeviceSelfPlay.file_to)" if not self._filers else
                               "several actors file into this buffer: name the filer (what attach_filer returned)")
        return self._filers[0]

    def _push_counters(self):
        counters = numpy.array([self.num_played_games, len(self.buffer), self.total_samples, self.num_played_steps],
                               dtype=numpy.int64)
        with torch.cuda.device(self.device):    # (the counters are the store's: any of its filers reaches them)
            self._check(self._lib.mzreplay_filer_set_counters(self._filers[0].handle, ptr(counters, _native.c_i64_p),
                                                              self._stream()))

    def filer_begin(self, first_observations, first_to_play=None, filer=None):
        """Every env of the filing actor starts a game: device tensors f32 [E, ...] and int32 [E] (None: player 0)."""
        filer = self._the_filer(filer)
        assert first_observations.is_cuda and first_observations.dtype == torch.float32 and first_observations.is_contiguous()
        assert first_observations.numel() == filer.num_envs * self.C * self.H * self.W
        assert first_to_play is None or (first_to_play.is_cuda and first_to_play.dtype == torch.int32
                                         and first_to_play.numel() == filer.num_envs)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_filer_begin(filer.handle, first_observations.data_ptr(),
                                                       None if first_to_play is None else first_to_play.data_ptr(),
                                                       self._stream()))

    def filer_file(self, moves, filer=None):
        """Queue the filing of a move batch (a _native.MzReplayFileMoves of device pointers) on the current stream.  The
        batch's games take the ids behind those of the filer_file call made before this one, through whichever filer."""
        filer = self._the_filer(filer)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_filer_file(filer.handle, ctypes.byref(moves), self._stream()))
        filer.pending = True

    @property
    def filing_pending(self):
        """A move batch was filed on the device (filer_file) and sync_filing has not fetched its games yet."""
        return any(f.pending for f in self._filers) or bool(self._unbooked)

    def filer_lengths(self, filer=None):
        """Moves played so far in every env's running game (int32 [E]; waits for the device)."""
        filer = self._the_filer(filer)
        out = numpy.zeros(filer.num_envs, dtype=numpy.int32)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_filer_lengths(filer.handle, ptr(out, c_i32_p), self._stream()))
        return out

    def _sync_if_pending(self):
        if self.filing_pending:
            self.sync_filing()

    def _sync_filer(self, filer, counters):
        """mzreplay_filer_sync_ids of one filer: its new games as host arrays, the store's counters into `counters`; with
        them the games' outcome records (None from a filer that reports none)."""
        n = ctypes.c_int32()
        env_p, len_p, id_p = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        filer.pending = False
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_filer_sync_ids(filer.handle, ctypes.byref(n), ctypes.byref(env_p), ctypes.byref(len_p),
                                                          ctypes.byref(id_p), ptr(counters, _native.c_i64_p), self._stream()))
        count = n.value

        def arr(p, ctype, dtype):
            if count == 0:
                return numpy.zeros(0, dtype=dtype)
            return numpy.ctypeslib.as_array(ctypes.cast(p, ctype), shape=(count,)).copy()
        filed = arr(env_p, c_i32_p, numpy.int32), arr(len_p, c_i32_p, numpy.int32), arr(id_p, _native.c_i64_p, numpy.int64)
        records = None
        if filer.outcomes:
            n_out, out_p = ctypes.c_int32(), ctypes.c_void_p()
            self._check(self._lib.mzreplay_filer_sync_outcomes(filer.handle, ctypes.byref(n_out), ctypes.byref(out_p)))
            assert n_out.value == count, "the filer's outcome list left its game list"
            records = numpy.zeros(count, dtype=_native.GAME_OUTCOME_DTYPE)
            if count:
                ctypes.memmove(records.ctypes.data, out_p.value, records.nbytes)
        return filed, records

    def sync_filing(self, shared_storage=None):
        """The games filed on the device since the last sync join the host bookkeeping: `buffer` entries (length,
        history=None), num_played_games / num_played_steps / total_samples from the device counters and, for host-side
        prioritised sampling, the new games' initial priorities.  Every filer with a filing pending is synced, the new
        games of all of them are merged by ascending id and booked once, in id order, against the counters read after the
        last sync; each filer's (env_index, length, game_id) wait in it for its owner (DeviceFiler.take_filed).  With one
        filer on the store, returns that filer's (env_index, length, game_id) host arrays; with several, None.
        Small and blocking: 16 bytes per game come back.
        A filer whose device error word is set fails its sync with the word's message, which is raised here: nothing is
        booked then (the counters already count the games that filer keeps for its next sync), what the other filers
        handed over waits, and the following sync_filing books it all."""
        self._sync_filers(shared_storage)
        return self._filers[0].take_filed() if len(self._filers) == 1 else None

    def _sync_filers(self, shared_storage=None):
        if not self._filers:
            raise RuntimeError("sync_filing: no actor files into this buffer (DeviceSelfPlay.file_to)")
        counters = numpy.zeros(4, dtype=numpy.int64)
        synced, failure = self._unbooked, None
        self._unbooked = []
        for filer in [f for f in self._filers if f.pending or f.refused] or self._filers[:1]:
            try:
                filer.refused = False
                synced.append((filer, *self._sync_filer(filer, counters)))
            except RuntimeError as error:
                filer.refused = True
                failure = failure or error
        if failure is not None:
            self._unbooked = synced
            raise failure
        for filer, filed, records in synced:
            filer._filed.append(filed)
            if records is not None:
                filer._filed_outcomes.append(records)
        lengths = numpy.concatenate([filed[1] for _, filed, _ in synced]) if synced else numpy.zeros(0, dtype=numpy.int32)
        ids = numpy.concatenate([filed[2] for _, filed, _ in synced]) if synced else numpy.zeros(0, dtype=numpy.int64)
        order = numpy.argsort(ids, kind="stable")
        lengths, ids = lengths[order], ids[order]
        count = len(ids)
        if count:
            keep_from = max(0, count - self.capacity)            # the calls can finish more games than there are slots
            kept_ids, kept_len = ids[keep_from:].tolist(), lengths[keep_from:].tolist()
            if self.device_sampling:
                entries = [_DeviceEntry(self, gid, length=n_moves, history=None) for gid, n_moves in zip(kept_ids, kept_len)]
            else:
                entries = [dict(length=n_moves, history=None) for n_moves in kept_len]
                if self.config.PER:
                    slots = numpy.ascontiguousarray(numpy.asarray(kept_ids) % self.capacity, dtype=numpy.int32)
                    pri = numpy.zeros((len(kept_ids), self.L), dtype=numpy.float32)
                    game_pri = numpy.zeros(len(kept_ids), dtype=numpy.float32)
                    with torch.cuda.device(self.device):
                        self._check(self._lib.mzreplay_filer_priorities(self._filers[0].handle, len(kept_ids),
                                                                        ptr(slots, c_i32_p), ptr(pri, c_f32_p),
                                                                        ptr(game_pri, c_f32_p), self._stream()))
                    for g, entry in enumerate(entries):
                        entry["priorities"] = pri[g, : kept_len[g]].copy()
                        entry["game_priority"] = game_pri[g]
            self.buffer.update(zip(kept_ids, entries))
            oldest = int(counters[0]) - int(counters[1])
            for gid in [g for g in itertools.takewhile(lambda g: g < oldest, self.buffer)]:
                del self.buffer[gid]
        self.num_played_games, stored, self.total_samples, self.num_played_steps = (int(v) for v in counters)
        assert stored == len(self.buffer), "the device filer's game count left the host's"
        if shared_storage:
            shared_storage.set_info("num_played_games", self.num_played_games)
            shared_storage.set_info("num_played_steps", self.num_played_steps)

    def download_games(self, game_ids):
        """Stored games read back from the device as a self_play.PackedGames (rows max_moves wide; rewards float64 as the
        store holds them; env_index -1: the store does not keep it)."""
        from .self_play import PackedGames
        self._sync_if_pending()
        game_ids = [int(g) for g in game_ids]
        for gid in game_ids:
            if gid not in self.buffer:
                raise KeyError(f"game {gid} is not in the buffer")
        n = len(game_ids)
        slots = numpy.ascontiguousarray([self._slot(g) for g in game_ids], dtype=numpy.int32)
        lengths = numpy.zeros(n, dtype=numpy.int32)
        obs = numpy.zeros((n, self.L + 1, self.C, self.H, self.W), dtype=numpy.float32)
        act = numpy.zeros((n, self.L + 1), dtype=numpy.int32)
        rew = numpy.zeros((n, self.L + 1), dtype=numpy.float64)
        tp = numpy.zeros((n, self.L + 1), dtype=numpy.int32)
        cv = numpy.zeros((n, self.L, self.A), dtype=numpy.float64)
        rv = numpy.zeros((n, self.L), dtype=numpy.float64)
        if n:
            with torch.cuda.device(self.device):
                self._check(self._lib.mzreplay_read_games(self._h, n, ptr(slots, c_i32_p), ptr(lengths, c_i32_p),
                                                          ptr(obs, c_f32_p), ptr(act, c_i32_p), ptr(rew, c_f64_p),
                                                          ptr(tp, c_i32_p), ptr(cv, c_f64_p), ptr(rv, c_f64_p), self._stream()))
        return PackedGames(env_index=numpy.full(n, -1, dtype=numpy.int32), length=lengths, observations=obs, actions=act,
                           rewards=rew, to_play=tp, child_visits=cv, root_values=rv)

    def game_outcomes(self, game_ids):
        """What stored games report (csrc/game_outcomes.h; include/mzreplay.h mzreplay_game_outcomes): a
        self_play.GameOutcomes for `game_ids`, computed on the device whichever way the games were stored (save_game,
        save_games, a device filer).  One launch, a wavefront per game, 40 bytes per game back; env_index is -1 (the store
        does not keep it)."""
        from .self_play import GameOutcomes
        self._sync_if_pending()
        game_ids = [int(g) for g in game_ids]
        for gid in game_ids:
            if gid not in self.buffer:
                raise KeyError(f"game {gid} is not in the buffer")
        n = len(game_ids)
        slots = numpy.ascontiguousarray([self._slot(g) for g in game_ids], dtype=numpy.int32)
        records = numpy.zeros(n, dtype=_native.GAME_OUTCOME_DTYPE)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_game_outcomes(self._h, n, ptr(slots, c_i32_p), records.ctypes.data, self._stream()))
        lengths = numpy.array([self.buffer[g]["length"] for g in game_ids], dtype=numpy.int32)
        return GameOutcomes.from_records(numpy.full(n, -1, dtype=numpy.int32), lengths, game_ids, records)

    # ---- sampling (replay_buffer.py:135-195) -----------------------------------------------------------
    def sample_game(self, force_uniform=False):
        self._sync_if_pending()
        game_prob = None
        if self.config.PER and not force_uniform:
            game_probs = numpy.array([e["game_priority"] for e in self.buffer.values()], dtype="float32")
            game_probs /= numpy.sum(game_probs)
            game_index = self.rng.choice_p(game_probs)
            game_prob = game_probs[game_index]
        else:
            game_index = self.rng.choice(len(self.buffer))
        game_id = self.num_played_games - len(self.buffer) + game_index
        return game_id, self.buffer[game_id], game_prob

    def sample_n_games(self, n_games, force_uniform=False):
        self._sync_if_pending()
        ids = list(self.buffer.keys())
        if self.config.PER and not force_uniform:
            game_probs = numpy.array([self.buffer[g]["game_priority"] for g in ids], dtype="float32")
            game_probs /= numpy.sum(game_probs)
            prob_of = dict(zip(ids, game_probs))
            selected = [ids[i] for i in self.rng.choice_p_many(game_probs, n_games)]
        else:
            prob_of = {}
            selected = [ids[self.rng.choice(len(ids))] for _ in range(n_games)]
        return [(g, self.buffer[g], prob_of.get(g)) for g in selected]

    def sample_position(self, entry, force_uniform=False):
        position_prob = None
        if self.config.PER and not force_uniform:
            position_index, position_prob = self.rng.choice_priorities(entry["priorities"])
        else:
            position_index = self.rng.choice(entry["length"])
        return position_index, position_prob

    # ---- the sampler's state (device_sampling=True) ---------------------------------------------------
    def load_priorities(self, game_id, priorities):
        """Priorities of a stored game given by the caller (float32 [length]); its game priority becomes their maximum."""
        pri = numpy.ascontiguousarray(priorities, dtype=numpy.float32)
        assert len(pri) == dict.__getitem__(self.buffer[game_id], "length")
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_set_priorities(self._h, self._slot(game_id), int(game_id), ptr(pri, c_f32_p),
                                                          len(pri), self._stream()))

    def download_priorities(self, game_id):
        """(priorities float32 [length], game priority) of a stored game, read from the device (waits for it)."""
        row = numpy.zeros(self.L, dtype=numpy.float32)
        game_priority, stored_id = ctypes.c_float(), ctypes.c_int64()
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_get_priorities(self._h, self._slot(game_id), ptr(row, c_f32_p),
                                                          ctypes.byref(game_priority), ctypes.byref(stored_id), self._stream()))
        assert stored_id.value == game_id, "the slot holds another game"
        return row[: dict.__getitem__(self.buffer[game_id], "length")].copy(), numpy.float32(game_priority.value)

    def sampler_state(self):
        """The batch sampler's stream as numpy.random.get_state() gives it."""
        key = numpy.zeros(624, dtype=numpy.uint32)
        pos = ctypes.c_int32()
        self._check(self._lib.mzreplay_sampler_get_rng(self._h, ptr(key, _native.c_u32_p), ctypes.byref(pos)))
        return ("MT19937", key, pos.value, 0, 0.0)

    def set_sampler_state(self, state):
        key = numpy.ascontiguousarray(state[1], dtype=numpy.uint32)
        self._check(self._lib.mzreplay_sampler_set_rng(self._h, ptr(key, _native.c_u32_p), int(state[2])))

    def _get_batch_device(self, out=None):
        B, dev = int(self.config.batch_size), self.device
        stacked = int(self.config.stacked_observations)
        game_ids = torch.empty(B, dtype=torch.int64, device=dev)
        slots = torch.empty(B, dtype=torch.int32, device=dev)
        positions = torch.empty(B, dtype=torch.int32, device=dev)
        absorbing = torch.empty((B, self.U1), dtype=torch.int32, device=dev)
        if out is None:
            out = dict(observations=torch.empty((B, self.C + stacked * (self.C + 1), self.H, self.W), dtype=torch.float32, device=dev),
                       actions=torch.empty((B, self.U1), dtype=torch.int64, device=dev),
                       values=torch.empty((B, self.U1), dtype=torch.float32, device=dev),
                       rewards=torch.empty((B, self.U1), dtype=torch.float32, device=dev),
                       policies=torch.empty((B, self.U1, self.A), dtype=torch.float32, device=dev),
                       weights=torch.empty(B, dtype=torch.float32, device=dev) if self.config.PER else None,
                       gradient_scales=torch.empty((B, self.U1), dtype=torch.float32, device=dev))
        for key, dtype, count in (("observations", torch.float32, B * (self.C + stacked * (self.C + 1)) * self.H * self.W),
                                  ("actions", torch.int64, B * self.U1), ("values", torch.float32, B * self.U1),
                                  ("rewards", torch.float32, B * self.U1), ("policies", torch.float32, B * self.U1 * self.A),
                                  ("gradient_scales", torch.float32, B * self.U1)) + \
                ((("weights", torch.float32, B),) if self.config.PER else ()):
            t = out[key]
            if not (t.is_cuda and t.dtype == dtype and t.numel() == count and t.is_contiguous()):
                raise ValueError(f"get_batch(out=...): {key} must be a contiguous {dtype} CUDA tensor of {count} elements")
        weights = out["weights"] if self.config.PER else None
        with torch.cuda.device(dev):
            self._check(self._lib.mzreplay_sample_batch(
                self._h, B, self.num_played_games - len(self.buffer), len(self.buffer), int(self.total_samples),
                1 if self.config.PER else 0, game_ids.data_ptr(), slots.data_ptr(), positions.data_ptr(),
                absorbing.data_ptr(), weights.data_ptr() if weights is not None else None, self._stream()))
            self._check(self._lib.mzreplay_make_batch_device(
                self._h, B, slots.data_ptr(), positions.data_ptr(), absorbing.data_ptr(), out["observations"].data_ptr(),
                out["actions"].data_ptr(), out["values"].data_ptr(), out["rewards"].data_ptr(), out["policies"].data_ptr(),
                out["gradient_scales"].data_ptr(), self._stream()))
        return DeviceIndexBatch(game_ids, slots, positions), (out["observations"], out["actions"], out["values"], out["rewards"],
                                                             out["policies"], weights, out["gradient_scales"])

    # ---- get_batch (replay_buffer.py:67-133) -----------------------------------------------------------
    def get_batch(self, out=None):
        """(index_batch, batch).  Host sampling: the reference's list of pairs and fp64 device targets.  Device sampling:
        a DeviceIndexBatch and float32 / int64 CUDA tensors, queued on the current stream without waiting; `out` (a dict
        with the trainer's keys: observations, actions, values, rewards, policies, weights, gradient_scales) receives
        them in place."""
        self._sync_if_pending()
        if self.device_sampling:
            return self._get_batch_device(out)
        if out is not None:
            raise ValueError("get_batch(out=...) needs device_sampling=True")
        B = self.config.batch_size
        index_batch, weight_batch = [], [] if self.config.PER else None
        slots = numpy.zeros(B, dtype=numpy.int32)
        positions = numpy.zeros(B, dtype=numpy.int32)
        absorbing = numpy.zeros((B, self.U1), dtype=numpy.int32)
        for b, (game_id, entry, game_prob) in enumerate(self.sample_n_games(B)):
            game_pos, pos_prob = self.sample_position(entry)
            # make_target draws numpy.random.choice(action_space) for every state past the end of the game
            for u in range(self.U1):
                if game_pos + u > entry["length"]:
                    absorbing[b, u] = self.config.action_space[self.rng.choice(self.A)]
            index_batch.append([game_id, game_pos])
            slots[b], positions[b] = self._slot(game_id), game_pos
            if self.config.PER:
                weight_batch.append(1 / (self.total_samples * game_prob * pos_prob))
        if self.config.PER:
            weight_batch = numpy.array(weight_batch, dtype="float32") / max(weight_batch)
        out = self.make_targets(slots, positions, absorbing)
        return index_batch, (out["observation"], out["action"], out["value"], out["reward"], out["policy"],
                             weight_batch, out["gradient_scale"])

    def make_targets(self, slots, positions, absorbing):
        """Device tensors of a batch of (slot, position) pairs: observation [B,C',H,W] f32, action [B,U+1] i64,
        value / reward / gradient_scale [B,U+1] f64, policy [B,U+1,A] f64."""
        B = len(slots)
        stacked = int(self.config.stacked_observations)
        dev = self.device
        out = dict(observation=torch.empty((B, self.C + stacked * (self.C + 1), self.H, self.W), dtype=torch.float32, device=dev),
                   action=torch.empty((B, self.U1), dtype=torch.int64, device=dev),
                   value=torch.empty((B, self.U1), dtype=torch.float64, device=dev),
                   reward=torch.empty((B, self.U1), dtype=torch.float64, device=dev),
                   policy=torch.empty((B, self.U1, self.A), dtype=torch.float64, device=dev),
                   gradient_scale=torch.empty((B, self.U1), dtype=torch.float64, device=dev))
        slots = numpy.ascontiguousarray(slots, dtype=numpy.int32)
        positions = numpy.ascontiguousarray(positions, dtype=numpy.int32)
        absorbing = numpy.ascontiguousarray(absorbing, dtype=numpy.int32)
        with torch.cuda.device(dev):
            self._check(self._lib.mzreplay_make_batch(
                self._h, B, ptr(slots, c_i32_p), ptr(positions, c_i32_p), ptr(absorbing, c_i32_p),
                out["observation"].data_ptr(), out["action"].data_ptr(), out["value"].data_ptr(), out["reward"].data_ptr(),
                out["policy"].data_ptr(), out["gradient_scale"].data_ptr(), self._stream()))
        self._keep = (slots, positions, absorbing)
        return out

    # ---- Reanalyse's two ends (replay_buffer.py:335-356) ------------------------------------------------
    def game_observations(self, game_id):
        """Stacked observations of every position of a stored game: CUDA tensor [n, C', H, W]."""
        self._sync_if_pending()
        n = self.buffer[game_id]["length"]
        stacked = int(self.config.stacked_observations)
        out = torch.empty((n, self.C + stacked * (self.C + 1), self.H, self.W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_game_observations(self._h, self._slot(game_id), n, out.data_ptr(), self._stream()))
        return out

    def set_reanalysed_values(self, game_id, values):
        """game_history.reanalysed_predicted_root_values = values (float32 [n], tensor or array)."""
        self._sync_if_pending()
        if game_id not in self.buffer:      # the game could have been removed since its selection
            return
        n = self.buffer[game_id]["length"]
        v = torch.as_tensor(values, dtype=torch.float32).reshape(-1).contiguous()
        assert v.numel() == n
        self._keep_values = v
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_set_reanalysed(self._h, self._slot(game_id), v.data_ptr(), n, self._stream()))
        self.buffer[game_id]["reanalysed"] = True

    # ---- Reanalyse in batches (include/mzreplay.h mzreplay_reanalyse_*) ----------------------------------
    def reanalyse_plan(self, n_games, game_ids=None):
        """Queue the plan of a pass of `n_games` draws (1..4096) on the current stream and return it (ReanalysePlan).
        game_ids None: drawn on the device, numpy.random.choice(len(buffer)) each, from the pass's own stream; else the
        caller's ids (each stored now), and the stream does not move.  An empty buffer gives a plan without rows."""
        self._sync_if_pending()
        n_games = int(n_games)
        if not 1 <= n_games <= 4096:
            raise ValueError("reanalyse_plan: n_games must be 1..4096")
        given = None
        if game_ids is not None:
            given = numpy.ascontiguousarray(game_ids, dtype=numpy.int64).reshape(-1)
            if len(given) != n_games:
                raise ValueError("reanalyse_plan: game_ids must hold n_games ids")
        plan = self._reanalyse_plans.get(n_games)
        if plan is None:
            dev = self.device
            plan = ReanalysePlan(n_games, torch.empty(n_games, dtype=torch.int64, device=dev),
                                 torch.empty(n_games, dtype=torch.int32, device=dev),
                                 torch.zeros(n_games + 1, dtype=torch.int32, device=dev), n_games * self.L)
            self._reanalyse_plans[n_games] = plan
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_reanalyse_plan(
                self._h, n_games, self.num_played_games - len(self.buffer), len(self.buffer), ptr(given, _native.c_i64_p),
                plan.game_ids.data_ptr(), plan.slots.data_ptr(), plan.row_start.data_ptr(), self._stream()))
        return plan

    def reanalyse_observations(self, plan, n_rows=None):
        """The stacked observation of every row of the plan, CUDA tensor [R, C', H, W] in row order: the input batch of
        initial_inference.  n_rows: R when the caller has read it already (else it is read here: 4 bytes, blocking)."""
        self._sync_if_pending()
        n_rows = plan.rows() if n_rows is None else int(n_rows)
        stacked = int(self.config.stacked_observations)
        out = torch.empty((n_rows, self.C + stacked * (self.C + 1), self.H, self.W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_reanalyse_observations(self._h, plan.n_games, plan.slots.data_ptr(),
                                                                  plan.row_start.data_ptr(), n_rows, out.data_ptr(),
                                                                  self._stream()))
        return out

    def reanalyse_store(self, plan, values):
        """values (float32 CUDA tensor [R], row order) become the reanalysed root values of the plan's games."""
        self._sync_if_pending()
        v = values.reshape(-1)
        if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
            raise ValueError("reanalyse_store: values must be a contiguous float32 CUDA tensor")
        if v.numel() == 0:
            return
        self._keep_values = v
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_reanalyse_store(self._h, plan.n_games, plan.slots.data_ptr(),
                                                           plan.row_start.data_ptr(), v.data_ptr(), self._stream()))

    def reanalyse_fc_configure(self, flat):
        """Describe config's fully-connected network to the store; `flat` (weights.FlatWeights) is the buffer the pass
        reads from then on -- a publish or a broadcast into it refreshes the network.  Raises what the library refuses."""
        cfg = self.config
        desc = _native.MzFcDesc()
        desc.observation_floats = self.C * self.H * self.W * (cfg.stacked_observations + 1) + cfg.stacked_observations * self.H * self.W
        desc.encoding_size = int(cfg.encoding_size)
        for i, layers in enumerate((cfg.fc_representation_layers, cfg.fc_dynamics_layers, cfg.fc_reward_layers,
                                    cfg.fc_policy_layers, cfg.fc_value_layers)):
            if len(layers) > 3:
                raise RuntimeError("mzreplay_reanalyse_fc_configure: layer sizes outside the supported range "
                                   "(<= 3 hidden layers per MLP, widths <= 256)")
            desc.n_hidden[i] = len(layers)
            for k, width in enumerate(layers):
                desc.hidden[i][k] = int(width)
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_reanalyse_fc_configure(self._h, ctypes.byref(desc), int(cfg.support_size),
                                                                  flat.flat.data_ptr(), int(flat.numel)))
        self._reanalyse_flat = flat

    def reanalyse_fc(self, plan):
        """The whole pass for the configured fully-connected network, one launch behind the plan; nothing comes back."""
        self._sync_if_pending()
        with torch.cuda.device(self.device):
            self._check(self._lib.mzreplay_reanalyse_fc(self._h, plan.n_games, plan.slots.data_ptr(),
                                                        plan.row_start.data_ptr(), self._stream()))

    def download_reanalysed(self, game_ids):
        """(values float32 [n, max_moves], has_values bool [n]) of stored games, read from the device (waits for it): the
        whole reanalysed row of each game's slot -- entries past the game's length are not the game's."""
        self._sync_if_pending()
        slots = numpy.ascontiguousarray([self._slot(int(g)) for g in game_ids], dtype=numpy.int32)
        values = numpy.zeros((len(slots), self.L), dtype=numpy.float32)
        has = numpy.zeros(len(slots), dtype=numpy.uint8)
        if len(slots):
            with torch.cuda.device(self.device):
                self._check(self._lib.mzreplay_read_reanalysed(self._h, len(slots), ptr(slots, c_i32_p), ptr(values, c_f32_p),
                                                               has.ctypes.data, self._stream()))
        return values, has.astype(bool)

    def reanalyse_state(self):
        """The pass's stream as numpy.random.get_state() gives it."""
        key = numpy.zeros(624, dtype=numpy.uint32)
        pos = ctypes.c_int32()
        self._check(self._lib.mzreplay_reanalyse_get_rng(self._h, ptr(key, _native.c_u32_p), ctypes.byref(pos)))
        return ("MT19937", key, pos.value, 0, 0.0)

    def set_reanalyse_state(self, state):
        key = numpy.ascontiguousarray(state[1], dtype=numpy.uint32)
        self._check(self._lib.mzreplay_reanalyse_set_rng(self._h, ptr(key, _native.c_u32_p), int(state[2])))

    # ---- priorities (replay_buffer.py:197-220) ---------------------------------------------------------
    def update_priorities(self, priorities, index_info):
        self._sync_if_pending()
        if self.device_sampling:
            dev = self.device
            if not isinstance(index_info, DeviceIndexBatch):
                pairs = numpy.asarray(index_info, dtype=numpy.int64).reshape(-1, 2)
                index_info = DeviceIndexBatch(torch.from_numpy(pairs[:, 0].copy()).to(dev), None,
                                              torch.from_numpy(pairs[:, 1].astype(numpy.int32)).to(dev))
            pri = torch.as_tensor(priorities, dtype=torch.float32, device=dev).contiguous()
            assert pri.shape == (len(index_info), self.U1), "priorities: [batch, num_unroll_steps + 1]"
            with torch.cuda.device(dev):
                self._check(self._lib.mzreplay_update_priorities(self._h, len(index_info), index_info.game_ids.data_ptr(),
                                                                 index_info.positions.data_ptr(), pri.data_ptr(),
                                                                 self._stream()))
            return
        for i in range(len(index_info)):
            game_id, game_pos = index_info[i]
            if next(iter(self.buffer)) <= game_id:
                entry = self.buffer[game_id]
                priority = priorities[i, :]
                start_index = game_pos
                end_index = min(game_pos + len(priority), len(entry["priorities"]))
                entry["priorities"][start_index:end_index] = priority[: end_index - start_index]
                entry["game_priority"] = numpy.max(entry["priorities"])


class Reanalyse:
    """Reanalyse (reference replay_buffer.py:297-361) against the device store.  `reanalyse_game`: the reference's loop
    body, one batched initial_inference over all positions of a sampled game, support_to_scalar, values written back.
    `reanalyse_games`: N games per pass, queued on one stream (module docstring)."""

    def __init__(self, initial_checkpoint, config, device=None, flat=None, max_rows=8192):
        """flat: the weights.FlatWeights the fully-connected pass reads (e.g. the actor's buffer `Trainer.publish` writes
        into); without one the model's own weights are flattened at the first pass and `model.set_weights` keeps
        reaching them (a buffer handed in is refreshed by whoever owns it).  max_rows: rows per
        initial_inference call on the torch path of `reanalyse_games`."""
        from . import models
        self._models = models
        self.config = config
        torch.manual_seed(self.config.seed)
        self.device = torch.device(device if device is not None else "cuda")
        self.model = models.MuZeroNetwork(self.config)
        self.model.set_weights(initial_checkpoint["weights"])
        self.model.to(self.device)
        self.model.eval()
        self.num_reanalysed_games = initial_checkpoint.get("num_reanalysed_games", 0)
        self.flat = flat
        self.max_rows = int(max_rows)
        self._fc_store = None            # (store, flat buffer) the FC pass is configured for
        self._fc_refused = None          # the library's message where it refused this network

    @torch.no_grad()
    def reanalyse_game(self, replay_buffer, game_id=None):
        """One pass of the reference's loop body; returns (game_id, values tensor)."""
        if game_id is None:
            game_id, _, _ = replay_buffer.sample_game(force_uniform=True)
        values = None
        if self.config.use_last_model_value:
            observations = replay_buffer.game_observations(game_id)
            values = self._models.support_to_scalar(self.model.initial_inference(observations)[0], self.config.support_size)
            values = values.reshape(-1).float()
            replay_buffer.set_reanalysed_values(game_id, values)
        self.num_reanalysed_games += 1
        return game_id, values

    def _fc_pass_ready(self, replay_buffer):
        """True when the HIP pass covers this network on this store (configured on first use).  The choice follows the
        network kind and shape alone: a shape the library refuses takes the torch path, its message is kept."""
        if self.config.network != "fullyconnected":
            return False
        if self._fc_store is not None and self._fc_store[0] is replay_buffer:
            return True
        if self._fc_refused is not None and self._fc_refused[0] is replay_buffer:
            return False
        if self.flat is None:
            from .weights import FlatWeights
            self.flat = FlatWeights(self.model)
        try:
            replay_buffer.reanalyse_fc_configure(self.flat)
        except RuntimeError as err:
            self._fc_refused = (replay_buffer, str(err))
            return False
        self._fc_store = (replay_buffer, self.flat)
        return True

    @torch.no_grad()
    def _pass_torch(self, replay_buffer, plan, max_rows=None):
        """The pass of a plan through the torch model (any network); returns the values (CUDA float32 [R]) or None."""
        rows = plan.rows()                                   # the pass's one host round trip
        if not rows:
            return None
        observations = replay_buffer.reanalyse_observations(plan, rows)
        step = int(max_rows if max_rows is not None else self.max_rows)
        values = torch.empty(rows, dtype=torch.float32, device=observations.device)
        for at in range(0, rows, step):
            logits = self.model.initial_inference(observations[at: at + step])[0]
            values[at: at + step] = self._models.support_to_scalar(logits, self.config.support_size).reshape(-1)
        replay_buffer.reanalyse_store(plan, values)
        return values

    @torch.no_grad()
    def reanalyse_games(self, replay_buffer, n_games, game_ids=None, max_rows=None):
        """A pass over `n_games` games (drawn uniformly on the device from the pass's own stream, or `game_ids`); every
        position of every game is evaluated once with the current weights and the values are written into the store.
        Returns the number of draws.  While the store is empty or use_last_model_value is false it only counts.

        Fully-connected networks the library admits: plan + one HIP launch on the flat weights -- no blocking call, no
        allocation, no host-side decision (the pass can be captured in a graph).  Any other network: plan -> ONE 4-byte
        readback of the row count -> stacked observations -> model.initial_inference in chunks of at most `max_rows`
        rows -> support_to_scalar -> store: one host round trip per PASS, where reanalyse_game makes several per game."""
        n_games = int(n_games)
        if not 1 <= n_games <= 4096:
            raise ValueError("reanalyse_games: n_games must be 1..4096")
        replay_buffer._sync_if_pending()
        if self.config.use_last_model_value and len(replay_buffer.buffer) > 0:
            plan = replay_buffer.reanalyse_plan(n_games, game_ids)
            if self._fc_pass_ready(replay_buffer):
                replay_buffer.reanalyse_fc(plan)
            else:
                self._pass_torch(replay_buffer, plan, max_rows)
        self.num_reanalysed_games += n_games
        return n_games

    def reanalyse(self, replay_buffer, shared_storage, max_games=None, games_per_pass=1):
        """The reference's loop without Ray: runs until shared_storage reports the end of training.  games_per_pass > 1:
        every turn is a `reanalyse_games` pass of that many games."""
        done = 0
        while shared_storage.get_info("training_step") < self.config.training_steps and not shared_storage.get_info("terminate"):
            self.model.set_weights(shared_storage.get_info("weights"))
            if games_per_pass == 1:
                self.reanalyse_game(replay_buffer)
            else:
                self.reanalyse_games(replay_buffer, games_per_pass)
            shared_storage.set_info("num_reanalysed_games", self.num_reanalysed_games)
            done += games_per_pass
            if max_games is not None and done >= max_games:
                break
