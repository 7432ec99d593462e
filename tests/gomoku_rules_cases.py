"""Fixture G25 (tests/golden/g25_gomoku_rules.npz; recorded from the reference by tests/golden/make_golden_gomoku.py
g25_gomoku_rules) as plain rows, shared by test_gomoku_rules_cpu.py and test_gpu_gomoku_rules.py.  Everything here is
computed once and handed out unchanged."""
import functools
import os

import numpy as np

import gomoku_rules_reference as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CELLS = model.CELLS
KINDS = ("complete", "blocked", "open", "leaving", "neighbour", "overline", "ballot")
# rows per kind, exactly (neighbour: one per walk through the bottom edge; ballot: one ply per empty cell of the eight
# boards): a fixture that lost rows fails
COUNTS = dict(complete=2520, blocked=2520, open=2520, leaving=232, neighbour=132, overline=644, ballot=134)
EMPTY_SETS = ([63], [64], [63, 64], [0, 120], [62, 63, 64, 65], list(range(64)), list(range(64, 121)), [56, 57, 120])


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "g25_gomoku_rules.npz"), allow_pickle=False)


def _cells_of(bits):
    """Packed bits per cell (uint8 [N, 16]) as a 0 / 1 table [N, 121]."""
    return np.unpackbits(bits, axis=1)[:, :CELLS]


def legal_table(empty):
    """A 0 / 1 table of empty cells [N, 121] as (legal lists int32 [N, 121] in ascending order, padded with -1; counts)."""
    n = empty.sum(axis=1).astype(np.int32)
    order = np.argsort(1 - empty.astype(np.int8), axis=1, kind="stable").astype(np.int32)
    return np.where(np.arange(CELLS)[None, :] < n[:, None], order, -1).astype(np.int32), n


@functools.lru_cache(maxsize=None)
def plies():
    """Every fixture ply as arrays over N rows: kind (index into KINDS), board int8 [N, 121] before the ply, player int8
    (+1 / -1), action int32, reward int32 and done bool from the reference's Game.step, finished_before bool (its
    is_finished of the board as handed in), legal int32 [N, 121] (-1 padded) and n_legal, the reference's legal list
    after the ply; start, direction, last, colour, variant, pair, fboard as the recorder describes them."""
    fx = fixture()
    assert tuple(str(k) for k in fx["kinds"]) == KINDS
    legal, n_legal = legal_table(_cells_of(fx["legal_after"]))
    assert np.array_equal(n_legal, fx["n_legal_after"])
    out = dict(kind=fx["kind"], board=fx["board"], player=fx["player"], action=fx["action"].astype(np.int32),
               reward=fx["reward"].astype(np.int32), done=fx["done"], finished_before=fx["finished_before"], legal=legal,
               n_legal=n_legal, start=fx["start"].astype(np.int32), direction=fx["direction"], last=fx["last"],
               colour=fx["colour"], variant=fx["variant"], pair=fx["pair"], fboard=fx["fboard"])
    for value in out.values():
        value.setflags(write=False)
    return out


def rows_of(*kinds):
    """The row numbers of the named kinds, in fixture order."""
    kind = plies()["kind"]
    return np.flatnonzero(np.isin(kind, [KINDS.index(k) for k in kinds]))


@functools.lru_cache(maxsize=None)
def ballot_boards():
    """The eight ballot-edge boards: (board int8 [8, 121], legal int32 [8, 121] -1 padded, n_legal [8]) -- the lists are
    the reference's legal_actions()."""
    fx = fixture()
    legal, n = legal_table(_cells_of(fx["fboard_legal"]))
    assert np.array_equal(n, fx["fboard_n_legal"])
    board = fx["fboard_board"]
    for value in (board, legal, n):
        value.setflags(write=False)
    return board, legal, n


@functools.lru_cache(maxsize=None)
def picks():
    """The random opponent's recorded draws: board (index into ballot_boards), seed, player, pick, slot, words, pos
    (numpy's stream position after the draw), reward and done of the ply."""
    fx = fixture()
    out = {k[len("pick_"):]: fx[k] for k in fx.files if k.startswith("pick_")}
    for value in out.values():
        value.setflags(write=False)
    return out


def observation_planes(boards, players):
    """model.observation over rows: float32 [N, 3, 11, 11]."""
    boards = np.asarray(boards).reshape(-1, model.SIZE, model.SIZE)
    turn = np.broadcast_to(np.asarray(players, np.float32).reshape(-1, 1, 1), boards.shape)
    planes = np.stack([boards == 1, boards == -1, turn], axis=1).astype(np.float32)
    spot = min(len(boards) - 1, 17)
    assert np.array_equal(planes[spot], model.observation(boards[spot].reshape(-1), int(np.asarray(players)[spot])))
    return planes


@functools.lru_cache(maxsize=None)
def model_plies():
    """The sound model's ply on every fixture row: (boards after int8 [N, 121], reward int32 [N], done bool [N],
    observation planes after float32 [N, 3, 11, 11])."""
    rows = plies()
    results = [model.ply(b, p, a) for b, p, a in zip(rows["board"].tolist(), rows["player"].tolist(), rows["action"].tolist())]
    after = np.array([r[0] for r in results], dtype=np.int8)
    reward = np.array([r[1] for r in results], dtype=np.int32)
    done = np.array([r[2] for r in results], dtype=bool)
    planes = observation_planes(after, -rows["player"].astype(np.int32))
    for value in (after, reward, done, planes):
        value.setflags(write=False)
    return after, reward, done, planes
