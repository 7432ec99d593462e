"""Helpers shared by the Gomoku tests (test_gomoku_cpu.py, test_gpu_gomoku.py): fixture G18 as boards, the hand-made
edge boards, and the names of the two trace files."""
import numpy as np

SIZE, CELLS = 11, 121
# (simulations, fixture): 12 searches of 30 simulations, one of the config's 400 (a file of its own: a trace row carries
# 121 priors and 121 logits per simulation)
TRACE_FILES = [(30, "g18_gomoku_traces"), (400, "g18_gomoku_traces_s400")]


def cell(r, c):
    return r * SIZE + c


def fixture_boards(fx):
    """(boards int8 [rows, 121], players int8 [rows] as +1 / -1) of every row of g18_gomoku_env."""
    obs = fx["obs"]
    boards = (obs[:, 0] - obs[:, 1]).astype(np.int8).reshape(len(obs), CELLS)   # planes: first player's stones, second's
    return boards, obs[:, 2, 0, 0].astype(np.int8)


def full_board_without_five(swap=1):
    """Colour of cell (r, c): first player's where (c + 2 r) mod 4 < 2 -- runs of two along rows and both diagonals,
    of one down the columns."""
    return np.array([swap if (c + 2 * r) % 4 < 2 else -swap for r in range(SIZE) for c in range(SIZE)], dtype=np.int8)


def edge_boards():
    """[(name, board int8[121] BEFORE the ply, player to move +1 / -1, action, finished after the ply)]: the ply is a
    quiet stone far from everything (or the last empty cell), so `finished` is a property of the board handed in."""
    def board(first=(), second=()):
        b = np.zeros(CELLS, dtype=np.int8)
        b[list(first)] = 1
        b[list(second)] = -1
        return b

    quiet = cell(10, 5)
    cases = [
        # consecutive cell numbers across a row end: (3,8) (3,9) (3,10) (4,0) (4,1)
        ("row_wrap_step1", board([cell(3, 8), cell(3, 9), cell(3, 10), cell(4, 0), cell(4, 1)]), -1, quiet, False),
        # cell numbers 12 apart, leaving the board on the right: (0,9) (1,10) | (3,0) (4,1) (5,2)
        ("row_wrap_step12", board(second=[9, 21, 33, 45, 57]), 1, quiet, False),
        # cell numbers 10 apart, leaving the board on the left: (2,1) (3,0) | (3,10) (4,9) (5,8)
        ("row_wrap_step10", board([23, 33, 43, 53, 63]), 1, quiet, False),
        # four at the right edge and the first cell of the next row
        ("four_at_right_edge", board([cell(6, 7), cell(6, 8), cell(6, 9), cell(6, 10), cell(7, 0)]), -1, quiet, False),
        # four at the bottom edge going down, four into the bottom corners diagonally
        ("four_at_bottom", board([cell(r, 3) for r in range(7, 11)], [cell(7 + i, 7 + i) for i in range(4)]), 1, cell(0, 0), False),
        ("six", board([cell(5, c) for c in range(2, 8)]), -1, quiet, True),
        # a five of the side NOT to move (the first player's; the second player moves elsewhere): finishes all the same
        ("five_of_side_not_to_move", board([cell(2 + i, 8 - i) for i in range(5)]), -1, quiet, True),
        ("five_of_side_to_move", board(second=[cell(r, 10) for r in range(6, 11)]), -1, cell(0, 0), True),
        ("five_into_corner_0_10", board([cell(0, c) for c in range(6, 11)]), 1, quiet, True),
        ("five_into_corner_10_0", board(second=[cell(6 + i, 4 - i) for i in range(5)]), 1, cell(0, 5), True),
    ]
    full = full_board_without_five()
    last = full.copy()
    last[cell(10, 10)] = 0                         # (c + 2 r) mod 4 = 2 there: the second player's cell
    cases.append(("last_cell_of_a_draw", last, -1, cell(10, 10), True))
    nearly = full.copy()
    nearly[[cell(10, 10), cell(0, 0)]] = 0
    cases.append(("two_cells_left_no_five", nearly, -1, cell(10, 10), False))
    return cases
