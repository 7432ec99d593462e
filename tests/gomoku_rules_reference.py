"""The rules of Gomoku once more, in plain Python over an explicit table of the board's 252 five-cell lines: an
independent model of csrc/gomoku_rules.h, the Gomoku kernels of csrc/env_kernels.hip and the host plugin
(games/gomoku.py).  Fixture G25 (recorded from the reference) is the judge of all of them; this model names what the
fixture covers (tests/golden/make_golden_gomoku.py lays its positions out with these tables, test_gomoku_rules_cpu.py
asserts the counts) and supplies the observation planes the fixture does not store.

Boards are flat sequences of 121 cells, cell = 11 * row + column, 0 empty, +1 first player, -1 second.  A line is five
cells inside the board, one step apart in one of the four directions the rules name; nothing here walks a bordered
board.

Every function that judges takes `defect=`: None is the sound model, a name from DEFECTS breaks one rule on purpose --
the fixture must tell each of them from the reference.
"""
import numpy as np

SIZE, CELLS = 11, 121
# (row, column) steps: down-left, down, down-right, right -- and the same steps in cell numbers
DIRECTIONS = ((1, -1), (1, 0), (1, 1), (0, 1))
CELL_STEPS = (10, 11, 12, 1)

DEFECTS = (
    "row_wraps",          # an unbordered walk in cell numbers: cell + k * step, wherever that lies in 0..120
    "no_down_left",       # the direction (1, -1) is never scanned
    "mover_only",         # only the colour of the side that just moved is scanned
    "exactly_five",       # a five with an equal stone before or behind it (an overline) does not finish
    "last_stone_only",    # only the lines through the stone just placed are scanned
    "second_half_blind",  # no line that starts in a cell >= 64 is scanned
    "draw_pays_nothing",  # the ply that fills the board without a five ends the game with reward 0
)


def _known(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    return defect


# ---- tables ------------------------------------------------------------------------------------------------------------
def walk(start, direction):
    """The in-board cells of the five-step walk from `start` in direction index `direction`, up to where it leaves."""
    r, c = divmod(start, SIZE)
    dr, dc = DIRECTIONS[direction]
    cells = []
    for k in range(5):
        x, y = r + k * dr, c + k * dc
        if not (0 <= x < SIZE and 0 <= y < SIZE):
            break
        cells.append(SIZE * x + y)
    return tuple(cells)


def unbordered_walk(start, direction, offset=0):
    """The cells start + k * step + offset (k = 0..4) that lie in 0..120: what a walk in cell numbers reaches."""
    cells = (start + k * CELL_STEPS[direction] + offset for k in range(5))
    return tuple(c for c in cells if 0 <= c < CELLS)


# every (start cell, direction): 252 whose walk stays on the board -- the lines -- and 232 whose walk leaves it
LINES = tuple((s, d, walk(s, d)) for s in range(CELLS) for d in range(4) if len(walk(s, d)) == 5)
LEAVING = tuple((s, d) for s in range(CELLS) for d in range(4) if len(walk(s, d)) < 5)
LINE_ID = {(s, d): i for i, (s, d, _) in enumerate(LINES)}
assert len(LINES) == 252 and len(LEAVING) == 232
# the walks that leave through the bottom edge: the three downward directions from rows 7..10
LEAVING_BOTTOM = tuple((s, d) for s, d in LEAVING if d < 3 and s // SIZE >= 7)
assert len(LEAVING_BOTTOM) == 132
# per cell: the ids of the lines through it
THROUGH = tuple(tuple(i for i, (_, _, cells) in enumerate(LINES) if cell in cells) for cell in range(CELLS))


def runs(lo=6, hi=11):
    """Every run of lo..hi cells in a line in each direction, as (start, direction, cells): 644 for 6..11."""
    out = []
    for d, (dr, dc) in enumerate(DIRECTIONS):
        for s in range(CELLS):
            r, c = divmod(s, SIZE)
            for n in range(lo, hi + 1):
                x, y = r + (n - 1) * dr, c + (n - 1) * dc
                if 0 <= x < SIZE and 0 <= y < SIZE:
                    out.append((s, d, tuple(SIZE * (r + k * dr) + c + k * dc for k in range(n))))
    return out


def extended(cells):
    """A line or run with the cell before its first and behind its last (where the board has them)."""
    (r0, c0), (r1, c1) = divmod(cells[0], SIZE), divmod(cells[1], SIZE)
    dr, dc = r1 - r0, c1 - c0
    rl, cl = divmod(cells[-1], SIZE)
    out = list(cells)
    for x, y in ((r0 - dr, c0 - dc), (rl + dr, cl + dc)):
        if 0 <= x < SIZE and 0 <= y < SIZE:
            out.append(SIZE * x + y)
    return out


def quiet_cell(board):
    """A cell for a ply that must change no verdict: the first corner (then the first cell) that is empty and has no
    stone among its up to eight neighbours -- a stone alone belongs to no five."""
    for cell in (0, SIZE - 1, CELLS - SIZE, CELLS - 1, *range(CELLS)):
        r, c = divmod(cell, SIZE)
        around = [SIZE * x + y for x in range(max(r - 1, 0), min(r + 2, SIZE)) for y in range(max(c - 1, 0), min(c + 2, SIZE))]
        if all(board[n] == 0 for n in around):
            return cell
    raise ValueError("no quiet cell")


# ---- the rules ---------------------------------------------------------------------------------------------------------
def _line_holds(board, cells, defect):
    colour = board[cells[0]]
    if colour == 0 or any(board[c] != colour for c in cells[1:]):
        return 0
    if defect == "exactly_five" and any(board[c] == colour for c in extended(cells)[5:]):
        return 0
    return colour


def five(board, mover=None, placed=None, defect=None):
    """Does any line hold five equal stones?  `mover` and `placed` (the colour and the cell of the ply just made) matter
    to the defects only."""
    _known(defect)
    if defect == "row_wraps":
        for s in range(CELLS):
            for d in range(4):
                cells = unbordered_walk(s, d)
                if len(cells) == 5 and board[s] != 0 and all(board[c] == board[s] for c in cells):
                    return True
        return False
    lines = LINES if defect != "last_stone_only" else [LINES[i] for i in THROUGH[placed]]
    for s, d, cells in lines:
        if defect == "no_down_left" and d == 0:
            continue
        if defect == "second_half_blind" and s >= 64:
            continue
        colour = _line_holds(board, cells, defect)
        if colour != 0 and (defect != "mover_only" or colour == mover):
            return True
    return False


def legal(board):
    return [i for i in range(CELLS) if board[i] == 0]


def to_play(player):
    return 0 if player == 1 else 1


def finished(board):
    """Is this position terminal, whoever moved last: a five of either colour, or no empty cell (the sound rules)."""
    return five(board) or not legal(board)


def ply(board, player, action, defect=None):
    """(board after, reward, done) of `player` (+1 / -1) placing a stone on cell `action`."""
    _known(defect)
    after = list(board)
    after[action] = player
    won = five(after, mover=player, placed=action, defect=defect)
    full = not legal(after)
    done = won or full
    reward = 1 if done else 0
    if defect == "draw_pays_nothing" and not won:
        reward = 0
    return after, reward, done


def observation(board, player):
    """Planes [first player's stones, second player's, side to move as +1 / -1] as float32 [3, 11, 11]."""
    b = np.asarray(board).reshape(SIZE, SIZE)
    return np.stack([b == 1, b == -1, np.full((SIZE, SIZE), player)]).astype(np.float32)


def numpy_pick(seed, cells):
    """numpy.random.seed(seed); numpy.random.choice(cells) -- and the generator's state afterwards."""
    rs = np.random.RandomState(seed)
    pick = int(rs.choice(cells))
    return pick, rs.get_state()
