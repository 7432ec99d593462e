"""Seeded scripts for the device frame stack (include/mzenv.h mzenv_stack_*, csrc/obs_stack.h) and the numpy model they are
checked against, which is GameHistory.get_stacked_observations of this package and nothing else.

A script is, per env and ply, what one self-play move hands to mzenv_stack_push: the action (-1 = the env was left
untouched), the done flag, and the observation the next search sees.  Frames are arbitrary float32 values (the stack only
copies), so every comparison is exact.  One ply in mid-script is a masked mzenv_stack_reset instead of a push.

Shapes: the device games' observation shapes, (1,1,4) CartPole, (3,3,3) TicTacToe / TwentyOne, (1,1,9) SimpleGrid;
n in {1, 2, 5}; E = 70, so a launch has a full 64-env group and a partial one.  Envs 0-3 are scripted by hand so that the
coverage test_obs_stack_cpu.py asserts holds for every (shape, n) whatever the seed draws elsewhere."""
import functools
import importlib

import numpy as np

SHAPES = ((1, 1, 4), (3, 3, 3), (1, 1, 9))
DEPTHS = (1, 2, 5)
E = 70
PLIES = 24
RESET_AT = 15                      # this ply is a masked reset, not a push
NUM_ACTIONS = 9


def case_seed(shape, n):
    return 1000 * SHAPES.index(tuple(shape)) + n


@functools.lru_cache(maxsize=None)
def script(shape, n):
    """dict(frames f32 [PLIES + 1, E, C, H, W] -- frames[0] the first observations, frames[t + 1] what the search after
    ply t sees --, actions i32 [PLIES, E], done u8 [PLIES, E], mask u8 [E] of the reset at ply RESET_AT)."""
    rs = np.random.RandomState(case_seed(shape, n))
    frames = rs.standard_normal((PLIES + 1, E) + tuple(shape)).astype(np.float32)
    actions = rs.randint(0, NUM_ACTIONS, size=(PLIES, E)).astype(np.int32)
    actions[rs.random_sample((PLIES, E)) < 0.15] = -1
    done = (rs.random_sample((PLIES, E)) < 0.15).astype(np.uint8)
    mask = (rs.random_sample(E) < 0.5).astype(np.uint8)
    # env 0: one game of n + 3 plies from the start (the ring wraps), ended by a done whose next observation must hold
    # none of its frames
    actions[: n + 4, 0] = np.arange(n + 4) % NUM_ACTIONS
    done[: n + 4, 0] = 0
    done[n + 3, 0] = 1
    # env 1: done on the very first ply of a game, twice in a row, then a game that ends before n frames exist
    actions[:3, 1] = (4, 5, 6)
    done[:3, 1] = (1, 1, 0)
    if n > 1:
        actions[3, 1], done[3, 1] = 7, 1
    # env 2: an untouched ply between two played ones of the same game
    actions[:3, 2] = (3, -1, 8)
    done[:3, 2] = 0
    # env 3: is reset in mid-game; env 4: keeps its frames through the reset
    mask[3], mask[4] = 1, 0
    actions[RESET_AT - 2: RESET_AT, 3:5] = 2
    done[RESET_AT - 2: RESET_AT, 3:5] = 0
    done[actions < 0] = 0                                   # an untouched env reports no done (include/mzenv.h mzenv_step)
    for t in range(PLIES):
        if t == RESET_AT:
            keep = mask == 0                                # a reset moves no position of the envs it leaves alone
        else:
            keep = actions[t] < 0                           # an untouched env shows the observation it showed before
        frames[t + 1, keep] = frames[t, keep]
    for a in (frames, actions, done, mask):
        a.setflags(write=False)
    return dict(frames=frames, actions=actions, done=done, mask=mask)


def game_history_class():
    return importlib.import_module("muzero-hypermodel_amd.self_play").GameHistory


def _new_game(GameHistory, frame):
    gh = GameHistory()
    gh.observation_history.append(frame)
    gh.action_history.append(0)
    return gh


@functools.lru_cache(maxsize=None)
def model(shape, n):
    """The stacked observations a correct stack emits: f32 [PLIES + 1, E, C + n (C + 1), H, W] -- [0] after the first
    reset of all envs, [t + 1] after ply t -- and per-(ply, env) bookkeeping for the coverage assertions: `held` i32
    [PLIES + 1, E], the previous frames the env's game has at that point."""
    GameHistory = game_history_class()
    sc = script(shape, n)
    frames, actions, done, mask = sc["frames"], sc["actions"], sc["done"], sc["mask"]
    games = [_new_game(GameHistory, frames[0, e]) for e in range(E)]
    c, h, w = shape
    want = np.zeros((PLIES + 1, E, c + n * (c + 1), h, w), dtype=np.float32)
    held = np.zeros((PLIES + 1, E), dtype=np.int32)

    def emit(t):
        for e in range(E):
            want[t, e] = np.asarray(games[e].get_stacked_observations(-1, n), dtype=np.float32)
            held[t, e] = len(games[e].observation_history) - 1
    emit(0)
    for t in range(PLIES):
        for e in range(E):
            nxt = frames[t + 1, e]
            if t == RESET_AT:
                if mask[e]:
                    games[e] = _new_game(GameHistory, nxt)
            elif actions[t, e] < 0:
                pass
            elif done[t, e]:
                games[e] = _new_game(GameHistory, nxt)
            else:
                games[e].action_history.append(int(actions[t, e]))
                games[e].observation_history.append(nxt)
        emit(t + 1)
    want.setflags(write=False)
    held.setflags(write=False)
    return want, held


def coverage(shape, n):
    """Which of the five situations a frame stack can get wrong some env of the script meets (all must be True)."""
    sc = script(shape, n)
    _, held = model(shape, n)
    actions, done = sc["actions"], sc["done"]
    played = actions >= 0
    pushes = [t for t in range(PLIES) if t != RESET_AT]
    ends = np.zeros((PLIES, E), dtype=bool)                 # ply t ends env e's game
    ends[pushes] = played[pushes] & (done[pushes] != 0)
    return dict(
        ring_wraps=bool((held > n).any()),
        # a game over with fewer than n frames (and, where n allows it, with some: zeros behind real frames)
        zeros_remain=bool((ends & (held[:-1] < n) & (held[:-1] > (0 if n > 1 else -1))).any()),
        done_after_frames=bool((ends & (held[:-1] > 0)).any()),
        untouched_between_played=bool(any(
            played[t - 1, e] and not done[t - 1, e] and not played[t, e] and played[t + 1, e]
            for e in range(E) for t in range(1, PLIES - 1) if RESET_AT not in (t - 1, t, t + 1))),
        done_on_first_ply=bool((ends & (held[:-1] == 0)).any()),
    )
