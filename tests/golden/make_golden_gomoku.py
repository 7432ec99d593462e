#!/usr/bin/env python3
"""Generate the Gomoku fixtures (G18, G25) under tests/golden/ by RUNNING the reference's games/gomoku.py.

Build-container only, like make_golden.py (whose helpers it imports and which stays as it is): the reference is
imported from its checkout, inputs and expected outputs are recorded as .npz files, and nothing but data is written.

    python tests/golden/make_golden_gomoku.py [--only env traces rules]

g25_gomoku_rules.npz -- the rules line by line: every one of the board's 252 five-cell lines completed, blocked and left
open, every walk that leaves the board, every overline, the boards at the edges of the two 64-cell halves of a legal
list, and the random opponent's draws on them (g25_gomoku_rules below describes the rows).

g18_gomoku_env.npz -- playouts of the reference's Game in G11's column layout (game, step, obs, legal, n_legal,
to_play, action, reward, done; Gomoku has no expert agent, so no `expert` column), one row per position, the terminal
one included.  `kind` names each game:
  * hand-steered games (the first player's stones named, the second player's scattered on cells of rows 8 and 10 unless said):
    five to the right / down / down-right / down-left in mid-board; five along row 0 into the corner (0,10); five
    down column 10 into the corner (10,10); five of the SECOND player; six in a row (the gap of XXX_XX filled);
    a full board without a five (colour of cell (r, c) = ((c + 2 r) mod 4 < 2), 61 + 60 stones, played in cell
    order per colour: finishes on ply 121 with reward 1);
    "wrap": runs that are consecutive only in cell numbering -- (3,8) (3,9) (3,10) (4,0) (4,1) [step 1],
    (0,9) (1,10) (3,0) (4,1) (5,2) [step 12], (2,1) (3,0) (3,10) (4,9) (5,8) [step 10] -- none of which is a five;
    the game goes on as a random playout.
  * 16 random playouts: actions drawn with numpy.random.RandomState(2025).choice(legal) (the steered "wrap" game
    continues from RandomState(2026)).
`cfg_*` / `config_*` scalars record the reference's MuZeroConfig for Gomoku field by field.

g18_gomoku_traces.npz -- MCTS.run traces in G5's layout (make_golden.trace_one) on positions of those playouts with
a REDUCED network (the Gomoku config with blocks = 1, channels = 16; synthetic weights, seed 0): 12 positions at 30
simulations -- early, middle and nearly full boards (legal sets of 121, 120, 116, 101, 100, 81, 80, 61, 60, 10, 6 and 3
cells), both players to move, temperatures 1 / 0.5 / 0.25.  Position p is searched from numpy seed 1800 + p.
Positions: plies 0, 1, 5 of random playout 0; plies 20, 21 / 40, 41 / 60, 61 of random playouts 1 / 2 / 3; the
full-board game at plies 111, 115, 118.
g18_gomoku_traces_s400.npz -- the same layout, one middle-game position (ply 31 of random playout 2, 90 legal cells)
at the config's own 400 simulations, numpy seed 1899.
A trace row carries 121 priors and 121 logits per simulation, which do not compress: the simulation counts and the
split into two files keep each file under half a megabyte.  `sim_maxucb` (the UCB maxima, which no test compares; a
[400, 401] float64 block in the second file) is left out of both.
"""
import argparse
import os
import sys

import numpy

import make_golden as mg

SIZE = 11


def cell(r, c):
    return r * SIZE + c


# the second player's harmless replies: far corners of the bottom rows, never two adjacent
SCATTER = [cell(10, 0), cell(10, 2), cell(10, 4), cell(10, 6), cell(8, 0), cell(8, 2)]


def interleave(first, second):
    """first[0], second[0], first[1], ... until `first` runs out (the second player moves last when both are as long)."""
    out = []
    for i, a in enumerate(first):
        out.append(a)
        if i < len(second):
            out.append(second[i])
    return out


def first_player_line(stones):
    return interleave(stones, SCATTER[: len(stones) - 1])


def draw_board_moves():
    first = [cell(r, c) for r in range(SIZE) for c in range(SIZE) if (c + 2 * r) % 4 < 2]
    second = [cell(r, c) for r in range(SIZE) for c in range(SIZE) if (c + 2 * r) % 4 >= 2]
    assert len(first) == 61 and len(second) == 60
    return interleave(first, second)


def steered_games():
    games = [
        ("five_right", first_player_line([cell(5, c) for c in range(3, 8)])),
        ("five_down", first_player_line([cell(r, 4) for r in range(2, 7)])),
        ("five_down_right", first_player_line([cell(1 + i, 1 + i) for i in range(5)])),
        ("five_down_left", first_player_line([cell(1 + i, 9 - i) for i in range(5)])),
        ("five_row0_corner", first_player_line([cell(0, c) for c in range(6, 11)])),
        ("five_column10_corner", first_player_line([cell(r, 10) for r in range(6, 11)])),
        ("five_second_player", interleave([cell(0, 0), cell(0, 2), cell(0, 4), cell(0, 6), cell(2, 0)],
                                          [cell(4 + i, 3 + i) for i in range(5)])),
        ("six", first_player_line([cell(5, 2), cell(5, 3), cell(5, 4), cell(5, 6), cell(5, 7), cell(5, 5)])),
        ("full_board_draw", draw_board_moves()),
    ]
    wrap_first = [cell(3, 8), cell(3, 9), cell(3, 10), cell(4, 0), cell(4, 1),      # step 1 across a row end
                  cell(0, 9), cell(1, 10), cell(3, 0), cell(5, 2),                 # step 12 (with (4,1))
                  cell(2, 1), cell(4, 9), cell(5, 8)]                              # step 10 (with (3,0), (3,10))
    wrap_second = [cell(10, 0), cell(10, 2), cell(10, 4), cell(10, 6), cell(10, 8), cell(8, 1), cell(8, 3), cell(8, 5),
                   cell(8, 7), cell(6, 0), cell(6, 4), cell(6, 6)]
    games.append(("wrap", interleave(wrap_first, wrap_second)))
    return games


def play_recorded(gomoku, g, kind, moves, rs, rows):
    """One game of the reference's Game: `moves` first, then rs.choice(legal) until it ends."""
    A = SIZE * SIZE
    game = gomoku.Game(g)
    obs = game.reset()
    t, done, action, reward = 0, False, -1, 0
    while True:
        legal = list(game.legal_actions())
        rows["game"].append(g); rows["step"].append(t); rows["action"].append(action)
        rows["reward"].append(reward); rows["done"].append(done)
        rows["to_play"].append(game.to_play()); rows["n_legal"].append(len(legal))
        rows["legal"].append(legal + [-1] * (A - len(legal)))
        rows["obs"].append(numpy.asarray(obs, dtype="float32"))
        if done:
            break
        if t < len(moves):
            action = int(moves[t])
            assert action in legal, (kind, t, action)
        else:
            assert rs is not None, f"steered game {kind} did not end with its last move"
            action = int(rs.choice(legal))
        obs, reward, done = game.step(action)
        t += 1
    assert rs is not None or t == len(moves), f"steered game {kind} ended early (ply {t} of {len(moves)})"
    return t


def full_config_scalars(config):
    out = {}
    for key, value in sorted(vars(config).items()):
        if key in ("results_path", "train_on_gpu"):      # a path with a time stamp; a property of the machine
            continue
        if value is None:
            value = "None"
        out["config_" + key] = numpy.array(value)
    out["config_temperatures"] = numpy.array([config.visit_softmax_temperature_fn(t) for t in (0, 4999, 5000, 7499, 7500, 10000)])
    return out


def g18_env(gomoku):
    rows = dict(game=[], step=[], action=[], reward=[], done=[], to_play=[], n_legal=[], legal=[], obs=[])
    kinds, lengths = [], []
    g = 0
    for kind, moves in steered_games():
        rs = numpy.random.RandomState(2026) if kind == "wrap" else None
        lengths.append(play_recorded(gomoku, g, kind, moves, rs, rows))
        kinds.append(kind)
        g += 1
    rs = numpy.random.RandomState(2025)
    for _ in range(16):
        lengths.append(play_recorded(gomoku, g, "random", [], rs, rows))
        kinds.append("random")
        g += 1
    arrays = {k: numpy.array(v) for k, v in rows.items()}
    arrays["legal"] = arrays["legal"].astype("int16")
    arrays["kind"] = numpy.array(kinds)
    arrays["length"] = numpy.array(lengths)
    config = gomoku.MuZeroConfig()
    arrays.update(mg.config_scalars(config))
    arrays.update(full_config_scalars(config))
    print("   gomoku games:", list(zip(kinds, lengths)))
    mg.save("g18_gomoku_env", **arrays)
    return arrays


def position(env, game, step):
    row = int(numpy.flatnonzero((env["game"] == game) & (env["step"] == step))[0])
    assert not env["done"][row]
    n = int(env["n_legal"][row])
    return env["obs"][row], [int(a) for a in env["legal"][row][:n]], int(env["to_play"][row])


def g18_traces(gomoku, models, self_play, env):
    config = gomoku.MuZeroConfig()
    config.blocks, config.channels = 1, 16
    model = mg.build_model(models, config, None, seed=0)
    kinds = [str(k) for k in env["kind"]]
    first_random = kinds.index("random")
    draw = kinds.index("full_board_draw")
    where = [(first_random, s) for s in (0, 1, 5)]
    where += [(first_random + 1 + i, s) for i in range(3) for s in ((20, 21), (40, 41), (60, 61))[i]]
    where += [(draw, s) for s in (111, 115, 118)]
    config.num_simulations = 30
    recs = []
    for p, (game, step) in enumerate(where):
        obs, legal, to_play = position(env, game, step)
        recs.append(mg.trace_one(models, self_play, config, model, obs, legal, to_play, 1800 + p,
                                 temperature=[1.0, 0.5, 1.0, 0.25][p % 4]))
    arrays = mg.stack_records(recs)
    arrays.pop("sim_maxucb")
    arrays.update(mg.config_scalars(config))
    arrays["position_game"] = numpy.array([g for g, _ in where])
    arrays["position_step"] = numpy.array([s for _, s in where])
    print("   gomoku traces: legal counts", arrays["n_legal"].tolist(), "to_play", arrays["to_play"].tolist(),
          "mean select depth", arrays["sim_depth"].mean())
    mg.save("g18_gomoku_traces", **arrays)
    config.num_simulations = 400
    obs, legal, to_play = position(env, first_random + 2, 31)
    big = mg.stack_records([mg.trace_one(models, self_play, config, model, obs, legal, to_play, 1899)])
    big.update(mg.config_scalars(config))
    big.pop("sim_maxucb")
    big["position_game"], big["position_step"] = numpy.array([first_random + 2]), numpy.array([31])
    print("   gomoku 400-simulation trace: legal", big["n_legal"].tolist(), "max depth", big["max_tree_depth"].tolist())
    mg.save("g18_gomoku_traces_s400", **big)


# G25: what the empty cells of the ballot-edge boards are (every other cell holds full_board_without_five's stone)
G25_EMPTY_SETS = ([63], [64], [63, 64], [0, 120], [62, 63, 64, 65], list(range(64)), list(range(64, 121)), [56, 57, 120])
G25_KINDS = ("complete", "blocked", "open", "leaving", "neighbour", "overline", "ballot")


def g25_gomoku_rules(gomoku):
    """The rules of Gomoku line by line.  The positions are laid out with the tables of tests/gomoku_rules_reference.py;
    every recorded verdict is the reference's own (Game.step, is_finished, legal_actions, get_observation), the env put
    into the position by assigning env.board and env.player.  One table of plies, `kind` naming the group (G25_KINDS):
      complete   per line (252), colour and last cell: variant 1 -- four stones, the mover places the fifth; variant 0 --
                 the five stands, the OTHER side plays a quiet stone.  2 520 rows, all finished with reward 1.
      blocked / open   the same 2 520 with the fifth cell holding the other colour / empty, and a quiet ply: none finished.
      leaving    per (start, direction) whose walk leaves the board (232): one colour on the walk's in-board cells and on
                 the cells start + k * step (step 10 / 11 / 12 / 1) inside 0..120.  None finished.
      neighbour  per walk leaving through the bottom edge (132): the cells start + k * step - 121 inside 0..120, what a
                 scan without a bottom border reads from the next board; `pair` = the walk's `leaving` row.
      overline   every run of 6..11 cells (644), colours alternating: variant 1 -- one cell of the run is the ply;
                 variant 0 -- the run stands and the other side plays a quiet stone.  All finished.
      ballot     boards without a five whose empty cells are G25_EMPTY_SETS[fboard]: a ply into each empty cell.
    Per row: board int8 [121] before the ply, player, action, reward, done, finished_before (is_finished of the board
    as handed in), the legal list after the ply as a bit per cell (the reference's list is ascending: asserted) and its
    length; start / direction / last / colour / variant say which line.  Observations are not stored: the recorder
    asserts that get_observation is the three planes of the board after and the side to move.  `pick_*`: the
    random opponent's draw -- numpy.random.seed(s); numpy.random.choice(legal) -- on the ballot boards with at most four
    empty cells, seeds searched until every slot of every board was drawn twice (and a draw of more than one word kept
    where one turned up): pick, slot, words consumed, stream position, and the reference's verdict of that ply."""
    tests_dir = os.path.dirname(mg.HERE)
    if tests_dir not in sys.path:
        sys.path.insert(0, tests_dir)
    import gomoku_rules_reference as model
    from gomoku_cases import full_board_without_five

    game = gomoku.Game()
    game.reset()
    rows = dict(kind=[], board=[], player=[], action=[], reward=[], done=[], finished_before=[], legal_after=[],
                n_legal_after=[], start=[], direction=[], last=[], colour=[], variant=[], pair=[], fboard=[])

    def put(board, player):
        game.env.board = numpy.array(board, dtype="int32").reshape(SIZE, SIZE)
        game.env.player = int(player)

    def record(kind, board, player, action, start=-1, direction=-1, last=-1, colour=0, variant=0, pair=-1, fboard=-1):
        put(board, player)
        before = bool(game.env.is_finished())
        put(board, player)
        obs, reward, done = game.step(int(action))
        after = [int(v) for v in game.env.board.reshape(-1)]
        legal = [int(a) for a in game.legal_actions()]
        assert legal == sorted(set(legal)) and legal == [i for i in range(SIZE * SIZE) if after[i] == 0]
        assert numpy.array_equal(numpy.asarray(obs, dtype="float32"), model.observation(after, -player))
        assert numpy.array_equal(numpy.asarray(game.env.get_observation()), numpy.asarray(obs))
        assert game.to_play() == model.to_play(-player)
        mask = numpy.zeros(128, dtype="uint8")
        mask[legal] = 1
        for key, value in (("kind", G25_KINDS.index(kind)), ("board", list(board)), ("player", player), ("action", action),
                           ("reward", reward), ("done", bool(done)), ("finished_before", before),
                           ("legal_after", numpy.packbits(mask)), ("n_legal_after", len(legal)), ("start", start),
                           ("direction", direction), ("last", last), ("colour", colour), ("variant", variant),
                           ("pair", pair), ("fboard", fboard)):
            rows[key].append(value)
        return reward, bool(done)

    def stones(cells, colour):
        board = [0] * (SIZE * SIZE)
        for c in cells:
            board[c] = colour
        return board

    # ---- complete, blocked, open: 252 lines x 2 colours x 5 last cells each
    for kind in ("complete", "blocked", "open"):
        for i, (start, direction, cells) in enumerate(model.LINES):
            for ci, colour in enumerate((1, -1)):
                for j in range(5):
                    variant = (i + ci + j) % 2
                    mover = colour if variant else -colour
                    board = stones(cells, colour)
                    if kind == "complete" and variant:
                        board[cells[j]] = 0
                        action = cells[j]
                    else:
                        if kind != "complete":
                            board[cells[j]] = -colour if kind == "blocked" else 0
                        action = model.quiet_cell(board)
                    verdict = record(kind, board, mover, action, start, direction, j, colour, variant)
                    assert verdict == ((1, True) if kind == "complete" else (0, False)), (kind, start, direction, colour, j)
    # ---- walks that leave the board, and what they would read from the next board
    leaving_row = {}
    for i, (start, direction) in enumerate(model.LEAVING):
        colour = 1 if i % 2 == 0 else -1
        board = stones(model.walk(start, direction) + model.unbordered_walk(start, direction), colour)
        leaving_row[(start, direction)] = len(rows["kind"])
        mover = colour if (i // 2) % 2 else -colour
        assert record("leaving", board, mover, model.quiet_cell(board), start, direction, -1, colour, (i // 2) % 2) == (0, False)
    for i, (start, direction) in enumerate(model.LEAVING_BOTTOM):
        pair = leaving_row[(start, direction)]
        colour = rows["colour"][pair]
        cells = model.unbordered_walk(start, direction, offset=-SIZE * SIZE)     # (none for a few down-left walks of row 7)
        board = stones(cells, colour)
        mover = colour if i % 2 else -colour
        assert record("neighbour", board, mover, model.quiet_cell(board), start, direction, -1, colour, i % 2, pair) == (0, False)
    # ---- overlines
    for i, (start, direction, cells) in enumerate(model.runs(6, 11)):
        colour = 1 if i % 2 == 0 else -1
        variant = (i // 2) % 2
        board = stones(cells, colour)
        if variant:
            action = cells[i % len(cells)]
            board[action] = 0
            mover = colour
        else:
            action, mover = model.quiet_cell(board), -colour
        assert record("overline", board, mover, action, start, direction, len(cells), colour, variant) == (1, True)
    # ---- ballot edges
    full = [int(v) for v in full_board_without_five()]
    fboards, flegal, fn = [], [], []
    for f, empty in enumerate(G25_EMPTY_SETS):
        board = list(full)
        for c in empty:
            board[c] = 0
        put(board, 1)
        assert not game.env.is_finished()
        legal = [int(a) for a in game.legal_actions()]
        assert legal == sorted(empty)
        mask = numpy.zeros(128, dtype="uint8")
        mask[legal] = 1
        fboards.append(board); flegal.append(numpy.packbits(mask)); fn.append(len(legal))
        for c in empty:
            record("ballot", board, full[c], c, fboard=f)
    counts = [rows["kind"].count(k) for k in range(len(G25_KINDS))]
    assert counts[:6] == [2520, 2520, 2520, 232, 132, 644] and counts[6] == sum(len(e) for e in G25_EMPTY_SETS), counts
    # ---- the random opponent's draw on the boards with at most four empty cells
    picks = dict(board=[], seed=[], player=[], pick=[], slot=[], words=[], pos=[], reward=[], done=[])
    seed = 25000
    for f, empty in enumerate(G25_EMPTY_SETS):
        if len(empty) > 4:
            continue
        seen, long_draw = [0] * len(empty), False
        while min(seen) < 2:
            seed += 1
            put(fboards[f], 1)
            legal = game.legal_actions()
            numpy.random.seed(seed)
            pick = int(numpy.random.choice(legal))
            pos = int(numpy.random.get_state()[2])
            words, slot = pos % 624, legal.index(pick)     # a fresh seed leaves the position at 624: the first word counts from 0
            if seen[slot] >= 2 and (long_draw or words < 2):
                continue
            seen[slot] += 1
            long_draw = long_draw or words >= 2
            player = 1 if len(picks["seed"]) % 2 == 0 else -1
            put(fboards[f], player)
            _, reward, done = game.step(pick)
            for key, value in (("board", f), ("seed", seed), ("player", player), ("pick", pick), ("slot", slot),
                               ("words", words), ("pos", pos), ("reward", reward), ("done", bool(done))):
                picks[key].append(value)
    print(f"   gomoku rules: rows per kind {dict(zip(G25_KINDS, counts))}, {len(picks['seed'])} opponent draws "
          f"(words {sorted(set(picks['words']))})")
    dtypes = dict(kind="int8", board="int8", player="int8", action="int16", reward="int8", done="bool",
                  finished_before="bool", legal_after="uint8", n_legal_after="int16", start="int16", direction="int8",
                  last="int8", colour="int8", variant="int8", pair="int32", fboard="int8")
    arrays = {k: numpy.array(v, dtype=dtypes[k]) for k, v in rows.items()}
    arrays.update(kinds=numpy.array(G25_KINDS), fboard_board=numpy.array(fboards, dtype="int8"),
                  fboard_legal=numpy.array(flegal, dtype="uint8"), fboard_n_legal=numpy.array(fn, dtype="int16"))
    pick_types = dict(board="int8", seed="int64", player="int8", pick="int16", slot="int16", words="int32", pos="int32",
                      reward="int8", done="bool")
    arrays.update({"pick_" + k: numpy.array(v, dtype=pick_types[k]) for k, v in picks.items()})
    mg.save_exact("g25_gomoku_rules", **arrays)        # (bytes that depend on the arrays alone: the file regenerates exactly)
    assert os.path.getsize(os.path.join(mg.HERE, "g25_gomoku_rules.npz")) < 1000000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    models, self_play = mg.import_reference()
    import torch
    torch.set_num_threads(1)
    import games.gomoku as gomoku
    if not args.only or "rules" in args.only:
        g25_gomoku_rules(gomoku)
    if args.only and not {"env", "traces"} & set(args.only):
        return
    env = g18_env(gomoku) if not args.only or "env" in args.only else numpy.load(mg.HERE + "/g18_gomoku_env.npz")
    if not args.only or "traces" in args.only:
        g18_traces(gomoku, models, self_play, env)


if __name__ == "__main__":
    sys.exit(main())
