#!/usr/bin/env python3
"""Generate the Gomoku fixtures (G18) under tests/golden/ by RUNNING the reference's games/gomoku.py.

Build-container only, like make_golden.py (whose helpers it imports and which stays as it is): the reference is
imported from its checkout, inputs and expected outputs are recorded as .npz files, and nothing but data is written.

    python tests/golden/make_golden_gomoku.py [--only env traces]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    models, self_play = mg.import_reference()
    import torch
    torch.set_num_threads(1)
    import games.gomoku as gomoku
    env = g18_env(gomoku) if not args.only or "env" in args.only else numpy.load(mg.HERE + "/g18_gomoku_env.npz")
    if not args.only or "traces" in args.only:
        g18_traces(gomoku, models, self_play, env)


if __name__ == "__main__":
    sys.exit(main())
