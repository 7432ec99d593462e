"""Fixture G24 (tests/golden/g24_tictactoe_rules.npz, g24_connect4_rules.npz; recorded from the reference by
tests/golden/make_golden.py g24_board_rules) as plain rows, shared by test_board_rules_cpu.py and
test_gpu_board_rules.py.  Everything here is computed once and handed out unchanged."""
import functools
import os

import numpy as np

import board_rules_reference as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


GAME_ID = {"tictactoe": 1, "connect4": 2}
SHAPE = {"tictactoe": (3, 3), "connect4": (6, 7)}
WIN_REWARD = {"tictactoe": 20, "connect4": 10}


@functools.lru_cache(maxsize=None)
def plies(name):
    """Every fixture ply of a game as arrays: board int8 [N, cells] before the ply, player int8 [N] (+1 / -1), action
    int32 [N], reward int32 [N] and done bool [N] from the reference's Game.step; Connect4 also legal int32 [N, 7]
    (-1 padded) and n_legal [N], the reference's legal list after the ply."""
    if name == "tictactoe":
        fx = load_golden("g24_tictactoe_rules")
        at = fx["ply_position"]
        out = dict(board=fx["board"][at], player=fx["player"][at], action=fx["ply_action"], reward=fx["ply_reward"],
                   done=fx["ply_done"])
    else:
        fx = load_golden("g24_connect4_rules")
        out = dict(board=fx["ply_board"], player=fx["ply_player"], action=fx["ply_action"], reward=fx["ply_reward"],
                   done=fx["ply_done"], legal=fx["ply_legal"], n_legal=fx["ply_n_legal"])
    for value in out.values():
        value.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expert_rows(name):
    """Every expert row of a game: board int8 [M, cells], player int8 [M], seed int64 [M], move int32 [M] (the
    reference's expert_agent() with numpy seeded `seed`)."""
    if name == "tictactoe":
        fx = load_golden("g24_tictactoe_rules")
        out = dict(board=fx["board"], player=fx["player"], seed=fx["seed"], move=fx["expert"])
    else:
        fx = load_golden("g24_connect4_rules")
        out = dict(board=fx["expert_board"], player=fx["expert_player"], seed=fx["expert_seed"], move=fx["expert_move"])
    for value in out.values():
        value.setflags(write=False)
    return out


def legal_of(name, board):
    return model.ttt_legal(board) if name == "tictactoe" else model.c4_legal(board)


@functools.lru_cache(maxsize=None)
def numpy_choices(name):
    """Per expert row what numpy does for the random draw: (pick, words consumed, generator state afterwards) of
    numpy.random.seed(seed); numpy.random.choice(legal)."""
    rows = expert_rows(name)
    out = []
    for board, seed in zip(rows["board"].tolist(), rows["seed"].tolist()):
        pick, state = model.numpy_pick(seed, legal_of(name, board))
        # a fresh seed leaves the position at 624; the first word regenerates the block and counts from 0
        out.append((pick, int(state[2]) % 624, state))
    return out


@functools.lru_cache(maxsize=None)
def model_plies(name):
    """The sound model's ply on every fixture row: (boards after int8 [N, cells], observation planes after float32
    [N, 3, rows, columns], legal lists after as a list of lists)."""
    rows = plies(name)
    ply = model.ttt_ply if name == "tictactoe" else model.c4_ply
    after = np.array([ply(b, p, a)[0] for b, p, a in zip(rows["board"].tolist(), rows["player"].tolist(),
                                                          rows["action"].tolist())], dtype=np.int8)
    planes = observation_planes(name, after, -rows["player"])
    legal = [legal_of(name, b) for b in after.tolist()]
    after.setflags(write=False)
    planes.setflags(write=False)
    return after, planes, legal


def observation_planes(name, boards, players):
    """model.observation over rows: float32 [N, 3, rows, columns]."""
    shape = SHAPE[name]
    boards = np.asarray(boards).reshape(-1, *shape)
    turn = np.broadcast_to(np.asarray(players, np.float32).reshape(-1, 1, 1), boards.shape)
    planes = np.stack([boards == 1, boards == -1, turn], axis=1).astype(np.float32)
    spot = min(len(boards) - 1, 17)
    assert np.array_equal(planes[spot], model.observation(boards[spot].reshape(-1), int(np.asarray(players)[spot]), shape))
    return planes
