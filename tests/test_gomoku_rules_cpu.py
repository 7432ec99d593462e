"""The rules of Gomoku against fixture G25, the parts that need no GPU.  G25 holds every one of the board's 252 five-cell
lines completed (by either colour, with each of its cells as the last stone), blocked and left open, every walk that
leaves the board, every overline, and the boards at the edges of the two 64-cell halves of a legal list; every verdict
in it is the reference's.  Held to it here: the plain model of gomoku_rules_reference.py (which also counts what the
fixture covers and must tell each of its named defects from the reference), the host plugin, and csrc/gomoku_rules.h
built for the host."""
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gomoku_rules_reference as model
from gomoku_cases import full_board_without_five
from gomoku_rules_cases import (CELLS, COUNTS, EMPTY_SETS, KINDS, ballot_boards, legal_table, model_plies, picks,
                                plies, rows_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


def gomoku():
    return importlib.import_module("muzero-hypermodel_amd.games.gomoku")


# ---- what the fixture holds -------------------------------------------------------------------------------------------
def test_g25_row_counts_lines_and_start_cells():
    """Exactly 2 520 completing plies, 2 520 blocked and 2 520 open fours, 232 walks that leave the board, 644 overlines
    (and 132 neighbour boards, 134 ballot plies): every one of the 252 lines with both colours and all five last cells,
    in both variants per (line, colour); every (start, direction) that leaves; every run of 6..11; every cell as a
    start cell.  The rows are what the recorder's layout says: stones on the line's cells, nothing else but the ply."""
    ply = plies()
    for k, name in enumerate(KINDS):
        assert int((ply["kind"] == k).sum()) == COUNTS[name], name
    assert len(ply["kind"]) == sum(COUNTS.values()) == 8702
    assert len(model.LINES) == 252 and len(model.LEAVING) == 232 and len(model.runs(6, 11)) == 644
    want = {(i, colour, j) for i in range(252) for colour in (1, -1) for j in range(5)}
    starts = set()
    for name in ("complete", "blocked", "open"):
        seen, variants = set(), {}
        for r in rows_of(name).tolist():
            s, d, j, colour, variant = (int(ply[k][r]) for k in ("start", "direction", "last", "colour", "variant"))
            cells = model.LINES[model.LINE_ID[(s, d)]][2]
            seen.add((model.LINE_ID[(s, d)], colour, j))
            variants.setdefault((s, d, colour), set()).add(variant)
            starts.add(s)
            board, mover, action = ply["board"][r], int(ply["player"][r]), int(ply["action"][r])
            assert mover == (colour if variant else -colour)
            on_line = board[list(cells)].tolist()
            fifth = {"complete": colour, "blocked": -colour, "open": 0}[name]
            if name == "complete" and variant:
                fifth = 0
                assert action == cells[j]                                    # the mover places the last stone
            else:
                assert action not in cells and board[action] == 0           # a quiet ply elsewhere
            assert on_line == [fifth if i == j else colour for i in range(5)]
            assert int((board != 0).sum()) == sum(v != 0 for v in on_line)   # nothing else on the board
        assert seen == want and len(seen) == 2520
        assert all(v == {0, 1} for v in variants.values()) and len(variants) == 504
    leaving = rows_of("leaving")
    assert sorted(zip(ply["start"][leaving].tolist(), ply["direction"][leaving].tolist())) == sorted(model.LEAVING)
    for r in leaving.tolist():
        s, d, colour = int(ply["start"][r]), int(ply["direction"][r]), int(ply["colour"][r])
        cells = set(model.walk(s, d)) | set(model.unbordered_walk(s, d))
        assert set(np.flatnonzero(ply["board"][r] == colour).tolist()) == cells and int((ply["board"][r] != 0).sum()) == len(cells)
        starts.add(s)
    wrapping = sum(len(model.unbordered_walk(s, d)) == 5 for s, d in model.LEAVING)
    assert wrapping == 96                                                    # walks a scan in cell numbers would call fives
    neighbour = rows_of("neighbour")
    assert sorted(zip(ply["start"][neighbour].tolist(), ply["direction"][neighbour].tolist())) == sorted(model.LEAVING_BOTTOM)
    for r in neighbour.tolist():
        s, d, colour, pair = (int(ply[k][r]) for k in ("start", "direction", "colour", "pair"))
        assert ply["kind"][pair] == KINDS.index("leaving") and (ply["start"][pair], ply["direction"][pair]) == (s, d)
        assert ply["colour"][pair] == colour
        assert np.flatnonzero(ply["board"][r] == colour).tolist() == sorted(model.unbordered_walk(s, d, offset=-CELLS))
    over = rows_of("overline")
    runs = model.runs(6, 11)
    for i, r in enumerate(over.tolist()):
        s, d, cells = runs[i]
        assert (int(ply["start"][r]), int(ply["direction"][r]), int(ply["last"][r])) == (s, d, len(cells))
        assert int(ply["colour"][r]) == (1 if i % 2 == 0 else -1)
        after = ply["board"][r].copy()
        after[ply["action"][r]] = ply["player"][r]
        assert (after[list(cells)] == ply["colour"][r]).all()
    assert set(ply["last"][over].tolist()) == set(range(6, 12)) and set(ply["variant"][over].tolist()) == {0, 1}
    assert starts == set(range(CELLS))
    # the recorded verdicts, by kind
    for name, verdict in (("complete", 1), ("blocked", 0), ("open", 0), ("leaving", 0), ("neighbour", 0), ("overline", 1)):
        rows = rows_of(name)
        assert (ply["reward"][rows] == verdict).all() and (ply["done"][rows] == bool(verdict)).all(), name
    assert set(np.unique(ply["reward"]).tolist()) == {0, 1} and np.array_equal(ply["reward"] == 1, ply["done"])


def test_g25_ballot_boards_and_draws():
    """The eight boards whose empty cells sit at the edges of the two 64-cell halves: each is full_board_without_five
    with exactly the listed cells empty, the recorded legal list is that list, there is one ply per empty cell, and
    the ply into the last empty cell ends the game as a draw that pays 1.  Every slot of every board with at most four
    empty cells was drawn by a recorded seed, and one draw took more than one word."""
    boards, legal, n = ballot_boards()
    ply, pick = plies(), picks()
    full = full_board_without_five()
    rows = rows_of("ballot")
    assert len(boards) == len(EMPTY_SETS) == 8
    for f, empty in enumerate(EMPTY_SETS):
        want = full.copy()
        want[empty] = 0
        assert np.array_equal(boards[f], want) and legal[f][: n[f]].tolist() == empty and n[f] == len(empty)
        mine = rows[ply["fboard"][rows] == f]
        assert ply["action"][mine].tolist() == empty and (ply["board"][mine] == boards[f]).all()
        assert (ply["done"][mine] == (len(empty) == 1)).all()
    small = [f for f, empty in enumerate(EMPTY_SETS) if len(empty) <= 4]
    drawn = set(zip(pick["board"].tolist(), pick["slot"].tolist()))
    assert drawn == {(f, k) for f in small for k in range(len(EMPTY_SETS[f]))} and len(drawn) == 13
    assert pick["words"].max() >= 2 and set(pick["player"].tolist()) == {1, -1}
    for f, seed, p, slot, words, pos in zip(*(pick[k].tolist() for k in ("board", "seed", "pick", "slot", "words", "pos"))):
        got, state = model.numpy_pick(seed, EMPTY_SETS[f])
        assert (got, int(state[2])) == (p, pos) and EMPTY_SETS[f][slot] == p and words == pos % 624


# ---- the model and the host plugin against every row ------------------------------------------------------------------
def test_sound_model_equals_every_g25_row():
    """Board after, reward, done and legal list of every row; the planes the model builds are the board after and the
    side to move (the recorder asserted the reference's get_observation against this same function)."""
    ply = plies()
    after, reward, done, planes = model_plies()
    want_after = ply["board"].copy()
    want_after[np.arange(len(want_after)), ply["action"]] = ply["player"]
    assert np.array_equal(after, want_after)
    assert np.array_equal(reward, ply["reward"]) and np.array_equal(done, ply["done"])
    legal, n = legal_table(after == 0)
    assert np.array_equal(legal, ply["legal"]) and np.array_equal(n, ply["n_legal"])
    assert all(model.legal(b) == l[:k].tolist() for b, l, k in zip(after[::97].tolist(), legal[::97], n[::97].tolist()))
    assert np.array_equal(planes[:, 0] - planes[:, 1], after.reshape(-1, 11, 11))
    assert (planes[:, 2] == -ply["player"].astype(np.float32)[:, None, None]).all()
    assert [model.finished(b) for b in ply["board"].tolist()] == ply["finished_before"].tolist()
    pick = picks()
    boards = ballot_boards()[0]
    for f, player, cell, r, d in zip(*(pick[k].tolist() for k in ("board", "player", "pick", "reward", "done"))):
        assert model.ply(boards[f].tolist(), player, cell)[1:] == (r, d)


def test_host_plugin_equals_every_g25_row():
    """games/gomoku.py put into every row's position: is_finished before, then step -- observation (the model's planes,
    float64 as the reference returns them), reward, done (values and Python types), legal list, to_play."""
    mod = gomoku()
    ply = plies()
    planes = model_plies()[3]
    env = mod.Gomoku()
    for r in range(len(ply["kind"])):
        env.board = ply["board"][r].reshape(11, 11).astype("int32")
        env.player = int(ply["player"][r])
        assert env.is_finished() == bool(ply["finished_before"][r]), r
        obs, reward, done = env.step(int(ply["action"][r]))
        assert type(reward) is int and type(done) is bool
        assert reward == ply["reward"][r] and done == bool(ply["done"][r]), r
        assert obs.dtype == np.float64 and np.array_equal(obs, planes[r]), r
        assert env.legal_actions() == ply["legal"][r][: ply["n_legal"][r]].tolist(), r
        assert env.to_play() == model.to_play(-int(ply["player"][r]))
    boards, legal, n = ballot_boards()
    for f in range(len(boards)):
        env.board = boards[f].reshape(11, 11).astype("int32")
        assert env.legal_actions() == legal[f][: n[f]].tolist() and not env.is_finished()


# ---- the cases have teeth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", model.DEFECTS)
def test_every_defect_is_caught_by_the_fixture(defect):
    """With one rule broken the model must disagree with the reference on at least one row: the count is printed, and
    the kinds of rows that catch each defect are the ones built for it."""
    ply = plies()
    wrong = []
    for r, (b, p, a) in enumerate(zip(ply["board"].tolist(), ply["player"].tolist(), ply["action"].tolist())):
        _, reward, done = model.ply(b, p, a, defect=defect)
        if reward != ply["reward"][r] or done != bool(ply["done"][r]):
            wrong.append(r)
    kinds = sorted({KINDS[ply["kind"][r]] for r in wrong})
    print(f"defect {defect}: {len(wrong)} of {len(ply['kind'])} rows differ from the reference, kinds {kinds}")
    assert len(wrong) > 0
    built_for = dict(row_wraps="leaving", no_down_left="complete", mover_only="complete", exactly_five="overline",
                     last_stone_only="complete", second_half_blind="complete", draw_pays_nothing="ballot")
    assert built_for[defect] in kinds
    with pytest.raises(ValueError):
        model.ply(ply["board"][0].tolist(), 1, 0, defect="no_such_defect")


# ---- the shared header built for the host -----------------------------------------------------------------------------
def test_shared_gomoku_rules_on_every_g25_board(tmp_path):
    """csrc/gomoku_rules.h + board_rules.h built for the host over every board of G25 before and after its ply:
    finished and the legal list are the reference's, the random opponent agrees with HostStream; the per-stone test on
    the bordered board counts exactly the stones the line table finds.  Then the recorded seeds: the opponent's move,
    the words it consumed and the stream position are numpy's."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gomoku_rules_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "gomoku_rules_check.cpp"), "-lm"], check=True)
    ply = plies()
    after = model_plies()[0]
    N = len(ply["kind"])
    rows = [(2500 + r, bool(ply["finished_before"][r]), ply["board"][r]) for r in range(N)]
    rows += [(12500 + r, bool(ply["done"][r]), after[r]) for r in range(N)]

    def five_starts(b):
        return sum(any(all(b[c] == b[s] for c in model.LINES[i][2]) for i in model.THROUGH[s] if model.LINES[i][0] == s)
                   for s in range(CELLS) if b[s] != 0)

    def feed(rows, *args):
        text = "\n".join(" ".join(map(str, [seed, int(fin), int((b == 0).sum())] + b.tolist() + np.flatnonzero(b == 0).tolist()))
                         for seed, fin, b in rows)
        proc = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=120)
        lines = proc.stdout.strip().splitlines()
        report = json.loads(lines[-1])
        assert proc.returncode == 0 and report["rows"] == len(rows), lines[-1]
        for key in ("finished_mismatches", "legal_mismatches", "random_mismatches", "stream_mismatches", "full_board_mismatches"):
            assert report[key] == 0, lines[-1]
        return report, lines[:-1]

    report, _ = feed(rows)
    full_after = int((ply["n_legal"] == 0).sum())
    assert report["full_boards"] == full_after == 2                         # the plies into {63} and {64}
    assert report["five_starts"] == sum(five_starts(b.tolist()) for _, _, b in rows) > 3000

    pick = picks()
    boards = ballot_boards()[0]
    report, lines = feed([(int(s), False, boards[f]) for f, s in zip(pick["board"].tolist(), pick["seed"].tolist())], "--picks")
    got = [tuple(int(v) for v in line.split()[1:]) for line in lines if line.startswith("pick ")]
    assert got == list(zip(pick["pick"].tolist(), pick["words"].tolist(), pick["pos"].tolist()))
    assert len(got) == len(pick["seed"]) >= 13
