"""Device-resident batched environments (include/mzenv.h): E games of one kind advance on the GPU with
one kernel per move instead of E host `Game.step` calls.  Same plugin semantics as the host `Game`
classes of this package (and therefore as the reference's games/*.py): observations, reward scaling,
legal-action order, `to_play`.  CartPole's physics is the restatement of games/cartpole.py: pinned to the
published equations, exact but for sin / cos within L ulps (tests/cartpole_reference.py); still unpinned against
gym itself, which is absent here.  get_state / set_state read and write its fp64 state.
"""
import ctypes

import numpy as np
import torch

from .. import _native

# (include/mzenv.h: 4 is no game and stays refused, the two numpy-only one-player games go on at 5)
GAME_IDS = {"cartpole": 0, "tictactoe": 1, "connect4": 2, "gomoku": 3, "twentyone": 5, "simple_grid": 6}
# the games' own lengths.  A TwentyOne player holds at least 1 and is done at 21: 20 plies at most.  SimpleGrid has no
# length of its own (an illegal move is a no-op ply): a value above any config.max_moves, so that the actors always hand
# the move limit to the env kernels
MAX_EPISODE_STEPS = {"cartpole": 500, "tictactoe": 9, "connect4": 42, "gomoku": 121, "twentyone": 20,
                     "simple_grid": 2 ** 31 - 1}
ONE_PLAYER_GAMES = ("cartpole", "twentyone", "simple_grid")   # every action legal in every state, nobody to play against
OPPONENT_KINDS = {"self": 0, "expert": 1, "random": 2}      # include/mzenv.h MZENV_OPPONENT_*
PAIRED_SLOTS = 3                                            # include/mzenv.h MZENV_PAIRED_SLOTS


class DeviceEnvs:
    def __init__(self, game, num_envs, seeds=None, device=None):
        self._lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceEnvs needs a HIP device; use the host Game plugins on CPU")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.game, self.E = game, int(num_envs)
        seeds = np.ascontiguousarray(np.arange(self.E) if seeds is None else seeds, dtype=np.int64) & 0xFFFFFFFF
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        handle = ctypes.c_void_p()
        rc = self._lib.mzenv_create(GAME_IDS[game], self.E, self.device.index, _native.ptr(seeds, _native.c_u32_p),
                                    ctypes.byref(handle))
        if rc != 0:
            raise RuntimeError(self._lib.mzenv_last_error(None).decode())
        self._h = handle
        a, p = ctypes.c_int32(), ctypes.c_int32()
        shape = (ctypes.c_int32 * 3)()
        self._lib.mzenv_shape(self._h, ctypes.byref(a), ctypes.byref(p), shape)
        self.A, self.players, self.observation_shape = a.value, p.value, tuple(shape)
        self.constant_legal_actions = game in ONE_PLAYER_GAMES     # every action legal in every state
        self.max_episode_steps = MAX_EPISODE_STEPS[game]
        with torch.cuda.device(self.device):
            self.obs = torch.zeros((self.E, *self.observation_shape), dtype=torch.float32, device=self.device)
            self.legal = torch.zeros((self.E, self.A), dtype=torch.int32, device=self.device)
            self.num_legal = torch.zeros(self.E, dtype=torch.int32, device=self.device)
            self.to_play = torch.zeros(self.E, dtype=torch.int32, device=self.device)
            self.reward = torch.zeros(self.E, dtype=torch.float32, device=self.device)
            self.done = torch.zeros(self.E, dtype=torch.uint8, device=self.device)
            self._actions = torch.zeros(self.E, dtype=torch.int32, device=self.device)
            # opponent mode: the action actually played and the stream words the opponent's choice consumed (u32 bits)
            self.played = torch.zeros(self.E, dtype=torch.int32, device=self.device)
            self.words = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        self.opponent = ("self", 0)
        self.max_moves = 0                                   # move limit (set_max_moves); 0 = the game's own rules only
        self.reset()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.mzenv_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mzenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_opponent(self, kind, muzero_player=0, engine=None):
        """Evaluation games (reference self_play.py:189-221): `kind` "expert" or "random" plays every side but
        `muzero_player`, drawing from `engine`'s per-env RNG streams (engine.BatchedMCTS: in a reference worker the
        opponent and the search share numpy's global generator); "self" switches the mode off.  While it is on,
        observe / advance report num_legal = 0 where the opponent is to move (the engine leaves such an env out of the
        search), step / advance play the opponent's move there whatever action comes in, and both fill `played` (the
        action actually played) and `words` (stream words consumed: hand their sums to engine.rng_consumed)."""
        if kind not in OPPONENT_KINDS:
            raise NotImplementedError('device envs play opponent "self", "expert" or "random" ("human": use SelfPlay)')
        if kind != "self" and self.game in ("twentyone", "simple_grid"):
            raise NotImplementedError(f"{self.game} is a one-player game: it has no opponent")
        if kind == "expert" and self.game == "gomoku":
            # (AbstractGame.expert_agent raises the same for a host Game: the reference's games/gomoku.py defines none)
            raise NotImplementedError('gomoku has no expert agent; its scripted opponent is "random"')
        key = pos = None
        if kind != "self":
            if engine is None:
                raise ValueError("set_opponent: the opponent draws from the search engine's streams; pass engine=")
            key, pos = engine.rng_streams()
        self._check(self._lib.mzenv_set_opponent(self._h, OPPONENT_KINDS[kind], int(muzero_player), key, pos))
        self.opponent = ("self", 0) if kind == "self" else (kind, int(muzero_player))
        self._opponent_engine = engine if kind != "self" else None    # (its streams must outlive the mode)

    def set_boards(self, boards, players):
        """Put the envs of a board game into given positions: boards int8 [E, cells] (0 / +1 / -1; connect four row 0
        = bottom; gomoku cell = 11 * row + column), players int8 [E] (+1 / -1 to move).  An env's ply count (game_moves) becomes its number of stones."""
        if self.game in ("twentyone", "simple_grid"):
            raise NotImplementedError(f"{self.game} has no board to set")
        boards = np.ascontiguousarray(boards, dtype=np.int8).reshape(self.E, -1)
        players = np.ascontiguousarray(players, dtype=np.int8).reshape(self.E)
        self._check(self._lib.mzenv_set_boards(self._h, boards.ctypes.data, players.ctypes.data))

    def get_state(self):
        """CartPole only: (state float64 [E, 4] in the order x, x_dot, theta, theta_dot, steps int32 [E]) as host arrays
        (copies; blocking)."""
        state, steps = np.empty((self.E, 4), np.float64), np.empty(self.E, np.int32)
        self._check(self._lib.mzenv_get_state(self._h, state.ctypes.data, steps.ctypes.data))
        return state, steps

    def set_state(self, state, steps=None):
        """CartPole only: every env's fp64 state becomes `state` [E, 4], stored as given (non-finite values included);
        `steps` int [E] becomes the ply counters, which the game's 500-step cap and the move limit read (None = the
        counters stay; negative = error).  The envs' streams are untouched.  Blocking."""
        state = np.ascontiguousarray(state, dtype=np.float64)
        if state.shape != (self.E, 4):
            raise ValueError(f"set_state: state must have shape ({self.E}, 4)")
        if steps is not None:
            steps = np.ascontiguousarray(steps, dtype=np.int32)
            if steps.shape != (self.E,):
                raise ValueError(f"set_state: steps must have shape ({self.E},)")
        self._check(self._lib.mzenv_set_state(self._h, state.ctypes.data, None if steps is None else steps.ctypes.data))

    def set_max_moves(self, max_moves):
        """Games end at `max_moves` plies (config.max_moves, reference self_play.py:129-131): the ply that brings an
        env's count to it -- the opponent's plies count too -- reports done = 1 whatever the game's own rules say, and
        advance() resets the env like any finished one; reward and observations are the ply's own.  0 = no limit.  With
        a limit set `done` means "the game is over", not "the position is terminal".  A host store: legal between any
        two calls, in effect from the next step / advance on.  `max_episode_steps` stays the game's own length."""
        self._check(self._lib.mzenv_set_max_moves(self._h, int(max_moves)))
        self.max_moves = int(max_moves)

    def game_moves(self):
        """Plies played so far in each env's current game (int32 [E] device tensor, a copy): zeroed by a reset, set to
        the number of stones by set_boards."""
        out = torch.empty(self.E, dtype=torch.int32, device=self.device)
        self._check(self._lib.mzenv_game_moves(self._h, out.data_ptr(), self._stream()))
        return out

    def reset(self, mask=None):
        """Game.reset() for the envs whose mask entry is non-zero (uint8 device tensor; None = all)."""
        self._keep = mask
        self._check(self._lib.mzenv_reset(self._h, None if mask is None else mask.data_ptr(), self._stream()))

    def step(self, actions, reward=None, done=None, played=None, words=None):
        """Game.step per env; `actions`: int array / tensor [E] (negative = leave that env alone).
        Returns (reward, done) device tensors: the caller's `reward` (f32 [E]) / `done` (u8 [E]) when given,
        otherwise this object's own buffers (valid until the next step).  In opponent mode (set_opponent) the played
        actions and consumed stream words go to `played` / `words` (int32 [E]; default: this object's buffers)."""
        if torch.is_tensor(actions) and actions.is_cuda and actions.dtype == torch.int32 and actions.is_contiguous():
            src = actions                                    # e.g. the search's own action buffer: no copy
        elif torch.is_tensor(actions):
            src = self._actions.copy_(actions.to(torch.int32), non_blocking=True)
        else:
            src = self._actions.copy_(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)), non_blocking=True)
        reward = self.reward if reward is None else reward
        done = self.done if done is None else done
        if self.opponent[0] != "self" or played is not None:
            played = self.played if played is None else played
            words = self.words if words is None else words
            self._keep_step = (src, reward, done, played, words)
            self._check(self._lib.mzenv_step_opponent(self._h, src.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                                      played.data_ptr(), words.data_ptr(), self._stream()))
            return reward, done
        self._keep_step = (src, reward, done)
        self._check(self._lib.mzenv_step(self._h, src.data_ptr(), reward.data_ptr(), done.data_ptr(), self._stream()))
        return reward, done

    def advance(self, actions, reward, done, obs_after, obs_next, played=None, words=None):
        """One self-play move of every env in one call: step, observation after the move (terminal ones
        included), reset of the finished envs, observation the next search sees.  All arguments are resident
        tensors (actions int32 [E]; outputs as in step / observe; played / words as in step)."""
        if self.opponent[0] != "self" or played is not None:
            played = self.played if played is None else played
            words = self.words if words is None else words
            self._keep_step = (actions, reward, done, obs_after, obs_next, played, words)
            self._check(self._lib.mzenv_advance_opponent(self._h, actions.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                                         obs_after.data_ptr(), obs_next.data_ptr(), self.legal.data_ptr(),
                                                         self.num_legal.data_ptr(), self.to_play.data_ptr(),
                                                         played.data_ptr(), words.data_ptr(), self._stream()))
            return obs_next
        self._keep_step = (actions, reward, done, obs_after, obs_next)
        self._check(self._lib.mzenv_advance(self._h, actions.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                            obs_after.data_ptr(), obs_next.data_ptr(), self.legal.data_ptr(),
                                            self.num_legal.data_ptr(), self.to_play.data_ptr(), self._stream()))
        return obs_next

    def reset_observation(self):
        """The observation Game.reset() gives in a board game, float32 [C, H, W]: an empty board with the first player
        (+1) to move -- the same position in every env, which is what lets a paired move, whose outputs show the position
        after its last ply, start a game's history in the middle of a move."""
        if self.players < 2:
            raise NotImplementedError(f"{self.game}: a reset deals from the env's own stream; there is no one reset observation")
        obs = np.zeros(self.observation_shape, dtype=np.float32)
        obs[2] = 1.0
        return obs

    def new_paired_outputs(self, *leading):
        """Zeroed device tensors for advance_paired, each with the slot axis in front of E (and `leading` in front of
        that): reward f32, done u8, obs_after f32, played i32, words i32 (u32 bits)."""
        lead, dev = tuple(leading) + (PAIRED_SLOTS, self.E), self.device
        return dict(reward=torch.zeros(lead, dtype=torch.float32, device=dev),
                    done=torch.zeros(lead, dtype=torch.uint8, device=dev),
                    obs_after=torch.zeros(lead + self.observation_shape, dtype=torch.float32, device=dev),
                    played=torch.zeros(lead, dtype=torch.int32, device=dev),
                    words=torch.zeros(lead, dtype=torch.int32, device=dev))

    def advance_paired(self, actions, reward, done, obs_after, obs_next, played, words):
        """One evaluation move of every env with the opponent's reply inside it, in one launch (include/mzenv.h
        mzenv_advance_paired): slot 0 is MuZero's ply (actions int32 [E]; < 0 or not MuZero's turn: empty), slots 1 and 2
        the opponent's plies while it is to move.  reward / done / obs_after / played / words carry the slot axis
        ([3, E, ...]: new_paired_outputs; played -1 = empty slot); obs_next and this object's legal / num_legal / to_play
        describe the position the next search sees: MuZero to move in every env.  All actions -1 = the settle launch:
        only the opponent's pending plies (openings after a reset when MuZero plays second)."""
        for name, t in (("reward", reward), ("done", done), ("obs_after", obs_after), ("played", played), ("words", words)):
            if t.shape[:2] != (PAIRED_SLOTS, self.E) or not t.is_contiguous():
                raise ValueError(f"advance_paired: {name} must be contiguous with shape [{PAIRED_SLOTS}, {self.E}, ...]")
        self._keep_step = (actions, reward, done, obs_after, obs_next, played, words)
        self._check(self._lib.mzenv_advance_paired(self._h, actions.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                                   obs_after.data_ptr(), obs_next.data_ptr(), self.legal.data_ptr(),
                                                   self.num_legal.data_ptr(), self.to_play.data_ptr(), played.data_ptr(),
                                                   words.data_ptr(), self._stream()))
        return obs_next

    def observe(self, obs=None):
        """(observations [E,C,H,W] f32, legal [E,A] i32, num_legal [E] i32, to_play [E] i32) device tensors;
        the observations go to the caller's `obs` buffer when given."""
        obs = self.obs if obs is None else obs
        self._check(self._lib.mzenv_observe(self._h, obs.data_ptr(), self.legal.data_ptr(),
                                            self.num_legal.data_ptr(), self.to_play.data_ptr(), self._stream()))
        return obs, self.legal, self.num_legal, self.to_play


class DeviceFrameStack:
    """The n previous frames of every env on the GPU (include/mzenv.h mzenv_stack_*): turns the environment kernels'
    plain observations into the search input of config.stacked_observations = n --
    GameHistory.get_stacked_observations(-1, n) of every env, [E, C + n (C + 1), H, W] -- with no host round trip.
    reset / push write into the caller's `out` tensor and return it; both are one launch on the current stream."""

    def __init__(self, num_envs, observation_shape, n, device=None):
        self._lib = _native.load()
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceFrameStack needs a HIP device; GameHistory.get_stacked_observations stacks on the host")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.E, self.n = int(num_envs), int(n)
        self.observation_shape = tuple(int(v) for v in observation_shape)
        c, h, w = self.observation_shape
        handle = ctypes.c_void_p()
        if self._lib.mzenv_stack_create(self.E, c, h, w, self.n, self.device.index, ctypes.byref(handle)) != 0:
            raise RuntimeError(self._lib.mzenv_stack_last_error(None).decode())
        self._h = handle
        self.stacked_shape = (c + self.n * (c + 1), h, w)
        assert self._lib.mzenv_stack_floats(self._h) == self.stacked_shape[0] * h * w

    def new_output(self, *leading):
        """A zeroed device tensor [*leading, E, C + n (C + 1), H, W] for reset / push to write."""
        return torch.zeros(tuple(leading) + (self.E,) + self.stacked_shape, dtype=torch.float32, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.mzenv_stack_last_error(self._h).decode())

    def _checked(self, t, dtype, shape, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"DeviceFrameStack: {what} must be a contiguous {dtype} device tensor of shape {shape}")
        return t

    def reset(self, obs, out, mask=None):
        """Envs whose mask entry is non-zero (uint8 [E] device tensor; None = all) forget their frames; `out` becomes
        every env's stacked observation with `obs` [E, C, H, W] as the current frame."""
        plain, stacked = (self.E,) + self.observation_shape, (self.E,) + self.stacked_shape
        self._checked(obs, torch.float32, plain, "obs")
        self._checked(out, torch.float32, stacked, "out")
        if mask is not None:
            self._checked(mask, torch.uint8, (self.E,), "mask")
        self._keep = (mask, obs, out)
        self._check(self._lib.mzenv_stack_reset(self._h, None if mask is None else mask.data_ptr(), obs.data_ptr(),
                                                out.data_ptr(), self._stream()))
        return out

    def push(self, obs_before, actions, done, obs_next, out):
        """One self-play move of every env: actions[e] < 0 = untouched (nothing pushed), else done[e] = the game is over
        (frames forgotten), else (obs_before[e], actions[e]) is pushed; `out` becomes [obs_next, frames newest first]."""
        plain, stacked = (self.E,) + self.observation_shape, (self.E,) + self.stacked_shape
        self._checked(obs_before, torch.float32, plain, "obs_before")
        self._checked(actions, torch.int32, (self.E,), "actions")
        self._checked(done, torch.uint8, (self.E,), "done")
        self._checked(obs_next, torch.float32, plain, "obs_next")
        self._checked(out, torch.float32, stacked, "out")
        self._keep = (obs_before, actions, done, obs_next, out)
        self._check(self._lib.mzenv_stack_push(self._h, obs_before.data_ptr(), actions.data_ptr(), done.data_ptr(),
                                               obs_next.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mzenv_stack_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
