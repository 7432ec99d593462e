"""The rules of TicTacToe and Connect4 once more, in plain Python over explicit line tables: an independent model of
csrc/board_rules.h, the board branch of csrc/env_kernels.hip and the host plugins (games/tictactoe.py,
games/connect4.py).  Fixture G24 (recorded from the reference) is the judge of all of them; this model counts what the
fixture covers (tests/golden/make_golden.py chooses positions with it, test_board_rules_cpu.py asserts the counts) and
supplies the observation planes and bookkeeping the fixture does not store.

Boards are flat sequences, 0 empty, +1 first player, -1 second: TicTacToe cell = 3 * row + column, Connect4 cell =
7 * row + column with row 0 at the bottom.

Every function takes `defect=`: None is the sound model, a name from DEFECTS breaks one rule on purpose -- the fixture
must tell each of them from the reference.
"""
import numpy as np

DEFECTS = (
    "horizontal_short",            # Connect4 horizontals start in columns 0..2 only (c + 3 < 6)
    "antidiagonal_not_from_row3",  # Connect4 anti-diagonals whose top stone sits in row 3 are missing (r - 3 > 0)
    "draw_reads_bottom_row",       # Connect4 "no legal action" looks at row 0 instead of row 5
    "expert_no_height_test",       # Connect4 expert: a row / diagonal gap counts wherever the stone would land
    "expert_returns_at_block",     # both experts: a block returns at once like an own line
    "expert_last_gap",             # both experts: the gap looked for from the line's last cell instead of its first, and
                                   # its index -- counted from there -- used as if counted from the first
)


def _known(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    return defect


# ---- line tables -------------------------------------------------------------------------------------------------------
# TicTacToe: the 8 lines in the order the expert reads them (row i, column i for i = 0..2, diagonal, anti-diagonal from
# the top right corner)
TTT_LINES = ((0, 1, 2), (0, 3, 6), (3, 4, 5), (1, 4, 7), (6, 7, 8), (2, 5, 8), (0, 4, 8), (2, 4, 6))

C4_ROWS, C4_COLS, C4_CELLS = 6, 7, 42
C4_KINDS = ("row", "column", "diagonal", "antidiagonal")


def _c4_line_table():
    """The 69 lines as (kind, cells): rows left to right, columns bottom up, diagonals from the bottom left, anti-diagonals
    from the bottom right (the order in which the expert's windows read them)."""
    lines = []
    for r in range(6):
        for c in range(4):
            lines.append(("row", tuple(7 * r + c + j for j in range(4))))
    for c in range(7):
        for r in range(3):
            lines.append(("column", tuple(7 * (r + j) + c for j in range(4))))
    for r in range(3):
        for c in range(4):
            lines.append(("diagonal", tuple(7 * (r + j) + c + j for j in range(4))))
    for r in range(3):
        for c in range(3, 7):
            lines.append(("antidiagonal", tuple(7 * (r + j) + c - j for j in range(4))))
    return tuple(lines)


C4_LINES = _c4_line_table()
C4_LINE_ID = {cells: i for i, (_, cells) in enumerate(C4_LINES)}
assert len(C4_LINES) == 69 and len(C4_LINE_ID) == 69
# per cell: (line id, index of the cell inside the line, the other three cells)
C4_THROUGH = tuple(tuple((i, cells.index(cell), tuple(x for x in cells if x != cell))
                         for i, (_, cells) in enumerate(C4_LINES) if cell in cells) for cell in range(42))


def c4_last_stone_cases():
    """The (line, last stone index) pairs gravity allows: any stone of a row or diagonal, the top stone of a column.
    Times two colours: 426 of 552."""
    return [(i, j) for i, (kind, _) in enumerate(C4_LINES) for j in range(4) if kind != "column" or j == 3]


def c4_lines(defect=None):
    """The lines the winner test knows."""
    _known(defect)
    keep = []
    for kind, cells in C4_LINES:
        if defect == "horizontal_short" and kind == "row" and cells[0] % 7 == 3:
            continue
        if defect == "antidiagonal_not_from_row3" and kind == "antidiagonal" and cells[3] // 7 == 3:
            continue
        keep.append(cells)
    return keep


def winner(board, colour, lines):
    return any(all(board[c] == colour for c in cells) for cells in lines)


def ttt_winner(board, colour, defect=None):
    return winner(board, colour, TTT_LINES)


def c4_winner(board, colour, defect=None):
    return winner(board, colour, c4_lines(defect))


# ---- bookkeeping -------------------------------------------------------------------------------------------------------
def ttt_legal(board):
    return [i for i in range(9) if board[i] == 0]


def c4_legal(board):
    return [c for c in range(7) if board[35 + c] == 0]


def to_play(player):
    return 0 if player == 1 else 1


def observation(board, player, shape):
    """Planes [first player's stones, second player's, side to move] as float32 [3, rows, columns]."""
    b = np.asarray(board).reshape(shape)
    return np.stack([b == 1, b == -1, np.full(shape, player)]).astype(np.float32)


def c4_heights(board):
    return [sum(board[7 * r + c] != 0 for r in range(6)) for c in range(7)]


# ---- the ply -----------------------------------------------------------------------------------------------------------
def ttt_ply(board, player, action, defect=None):
    """(board after, Game-level reward, done) of `player` (+1 / -1) taking cell `action`."""
    _known(defect)
    after = list(board)
    after[action] = player
    won = ttt_winner(after, player)
    return after, 20 if won else 0, won or not ttt_legal(after)


def c4_landing(board, column):
    """The cell a stone dropped into `column` comes to rest in (the column is not full)."""
    return next(7 * r + column for r in range(6) if board[7 * r + column] == 0)


def c4_ply(board, player, action, defect=None):
    """(board after, Game-level reward, done) of `player` (+1 / -1) dropping a stone into column `action`."""
    _known(defect)
    after = list(board)
    after[c4_landing(board, action)] = player
    won = c4_winner(after, player, defect)
    if defect == "draw_reads_bottom_row":
        nothing_legal = all(after[c] != 0 for c in range(7))
    else:
        nothing_legal = not c4_legal(after)
    return after, 10 if won else 0, won or nothing_legal


def c4_ply_events(board, player, action):
    """What the ply does to the lines through its cell: (completed, blocked) with completed = [(line id, index of this
    stone in the line)] for lines now holding four of `player`, blocked = [line id] for lines whose other three cells
    hold the other colour."""
    cell = c4_landing(board, action)
    completed, blocked = [], []
    for line, index, others in C4_THROUGH[cell]:
        total = board[others[0]] + board[others[1]] + board[others[2]]
        if total == 3 * player:
            completed.append((line, index))
        elif total == -3 * player:
            blocked.append(line)
    return completed, blocked


# ---- the experts -------------------------------------------------------------------------------------------------------
def _gap(values, defect):
    """Index of the gap the expert names in a line's values.  A line the experts act on (two equal stones in three cells,
    three in four) has exactly one empty cell, so WHICH gap is taken cannot go wrong; from which end it is counted can.
    The defect walks the line from its last cell and hands that count on as an index from the first."""
    if defect == "expert_last_gap":
        return next(j for j, v in enumerate(reversed(values)) if v == 0)
    return next(j for j, v in enumerate(values) if v == 0)


def ttt_expert(board, player, pick, defect=None):
    """The TicTacToe expert with `player` to move; `pick` is the random legal move it draws first.  Returns (move,
    findings): findings = [(line index in TTT_LINES, gap index, "own" | "block")] in reading order, up to the return."""
    _known(defect)
    move, findings = pick, []
    for index, cells in enumerate(TTT_LINES):
        values = [board[c] for c in cells]
        total = sum(values)
        if abs(total) != 2:
            continue
        gap = _gap(values, defect)
        own = total * player > 0
        findings.append((index, gap, "own" if own else "block"))
        move = cells[gap]
        if own or defect == "expert_returns_at_block":
            break
    return move, findings


def _c4_window_lines(k, l):
    """The ten lines of the 4 x 4 window with bottom row k and left column l, in reading order: (kind, index, cells)."""
    out = []
    for i in range(4):
        out.append(("row", i, tuple(7 * (k + i) + l + j for j in range(4))))
        out.append(("column", i, tuple(7 * (k + j) + l + i for j in range(4))))
    out.append(("diagonal", 0, tuple(7 * (k + j) + l + j for j in range(4))))
    out.append(("antidiagonal", 0, tuple(7 * (k + j) + l + 3 - j for j in range(4))))
    return out


C4_WINDOWS = tuple((k, l, tuple(_c4_window_lines(k, l))) for k in range(3) for l in range(4))
assert all(cells in C4_LINE_ID for _, _, lines in C4_WINDOWS for _, _, cells in lines)


def c4_expert(board, player, pick, defect=None):
    """The Connect4 expert with `player` to move; `pick` is the random legal column it draws first.  Returns (move,
    findings): findings = [(k, l, kind, index, gap, "own" | "block", passed)] in reading order, up to the return --
    window (bottom row k, left column l), line kind and its index inside the window, the gap's index along the line,
    whose line it is, and whether the height test passed (a column has none: always True).  Only a passed finding names
    a move."""
    _known(defect)
    heights = c4_heights(board)
    move, findings = pick, []
    for k, l, lines in C4_WINDOWS:
        for kind, index, cells in lines:
            values = [board[c] for c in cells]
            total = values[0] + values[1] + values[2] + values[3]
            if abs(total) != 3:
                continue
            gap = _gap(values, defect)
            cell = cells[gap]
            passed = kind == "column" or defect == "expert_no_height_test" or heights[cell % 7] == cell // 7
            own = total * player > 0
            findings.append((k, l, kind, index, gap, "own" if own else "block", passed))
            if passed:
                move = cell % 7
                if own or defect == "expert_returns_at_block":
                    return move, findings
    return move, findings


def first_effective(findings):
    """The first finding of c4_expert's list whose height test passed, or None."""
    return next((f for f in findings if f[6]), None)


def c4_finding_column(finding):
    k, l, kind, index, gap = finding[:5]
    cells = next(c for kd, ix, c in C4_WINDOWS[4 * k + l][2] if kd == kind and ix == index)
    return cells[gap] % 7


def numpy_pick(seed, legal):
    """numpy.random.seed(seed); numpy.random.choice(legal) -- and the generator's state afterwards."""
    rs = np.random.RandomState(seed)
    pick = int(rs.choice(legal))
    return pick, rs.get_state()
