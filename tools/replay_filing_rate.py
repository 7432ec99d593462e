#!/usr/bin/env python3
"""Moves per second of DeviceSelfPlay.play_moves with three sinks for the finished games, legs alternated in one process:

    none     no sink (what the README's "whole self-play loop" rates measure)
    host     on_games -> ReplayBuffer.save_games: env outputs downloaded, filed by host threads, padded, copied game by game
    device   file_to(replay_buffer): filed where the batch lies, 4 bytes per game come back (include/mzreplay.h)

    python tools/replay_filing_rate.py --config cartpole|tictactoe|tictactoe_fc|connect4|gomoku [--envs E] [--moves M]
                                       [--seconds 1.0] [--rounds 3] [--groups N] [--outcomes] [--out profiles/NAME.jsonl]

--outcomes adds a leg `device_outcomes` beside `device`: file_to(replay_buffer, outcomes=True), the filer also reports what
every finished game earned (csrc/game_outcomes.h) and the outcomes are taken after every batch, as a training loop does.

--groups N adds a pipelined leg for each sink (PipelinedDeviceSelfPlay with N groups on streams of their own, batches
prefetched: pipelined_none, pipelined_host, pipelined_device -- every group files into the one store through a filer of
its own) and runs them beside the one-actor `device` leg unless --legs says otherwise.

Every leg has an actor (and a store) of its own with the same weights and seeds; a round runs each leg for at least
--seconds after two warm-up batches; the clock is the host's, closed by a device synchronise.  One JSON line per leg with
every round's rate, their median and spread, and the algorithmic bytes one filing moves (computed from the shapes: what
the filer reads from the rings and writes into rows and slots) -- to set beside kernel times from a profiler run of this
script (rocprofv3 --kernel-trace --stats -- python tools/replay_filing_rate.py ...) and the HBM peak."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULTS = {"cartpole": (4096, 50), "tictactoe": (65536, 9), "tictactoe_fc": (32768, 8), "connect4": (1024, 8),
            "gomoku": (256, 8)}


def setup(name):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    game = name.split("_")[0]
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    if name == "tictactoe_fc":
        config.network, config.encoding_size = "fullyconnected", 8
        config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
    if game in ("connect4", "gomoku"):
        config.blocks, config.channels = 2, 32
    if game != "cartpole":
        config.num_simulations = 25
    config.temperature_threshold = None
    torch.manual_seed(0)
    return game, config, models.MuZeroNetwork(config).get_weights()


def filing_bytes(config, E, M, games, plies):
    """Bytes one filing moves for `plies` played env-moves that finish `games` games of plies / games moves each."""
    A, obs = len(config.action_space), 1
    for v in config.observation_shape:
        obs *= int(v)
    per_ply_read = 4 + 4 * A + 8 + 4 * A + 4 + 4 + 1 + 4 * obs          # action, visits, value sum, legal, count, reward, done, obs_after
    per_ply_write = 8 * A + 8 + 4 + 8 + 1 + 4 * obs                       # policy row, root value, action, reward, to_play, observation
    per_game_ply = 2 * (8 * A + 8 + 4 + 8 + 1 + 4 * obs)                  # row -> slot: read and written once more
    return plies * (per_ply_read + per_ply_write + per_game_ply) + games * 2 * 4 * obs   # + obs_next of every new game


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(DEFAULTS), default="cartpole")
    ap.add_argument("--envs", type=int)
    ap.add_argument("--moves", type=int)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--groups", type=int, default=1, help="N > 1: pipelined legs with N groups")
    ap.add_argument("--legs", help="default none,host,device; with --groups: pipelined_none,pipelined_host,pipelined_device,device")
    ap.add_argument("--outcomes", action="store_true", help="add the leg device_outcomes: the filer reports every game's outcome")
    ap.add_argument("--out")
    args = ap.parse_args()
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    game, config, weights = setup(args.config)
    E = args.envs or DEFAULTS[args.config][0]
    M = args.moves or DEFAULTS[args.config][1]
    config.replay_buffer_size = max(int(config.replay_buffer_size), 4 * E)
    legs = {}
    names = args.legs or ("none,host,device" if args.groups < 2 else "pipelined_none,pipelined_host,pipelined_device,device")
    if args.outcomes:
        names += ",device_outcomes"
    for leg in names.split(","):
        outcomes = leg.endswith("device_outcomes")
        pipelined, sink = leg.startswith("pipelined_"), "device" if outcomes else leg.split("_")[-1]
        if pipelined:
            if args.groups < 2:
                ap.error(f"leg {leg} needs --groups N with N > 1")
            actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 0, E, groups=args.groups)
        else:
            actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 0, E)
        store = None if sink == "none" else rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)
        on_games = None
        if sink == "host":
            on_games = store.save_games
        elif sink == "device":
            actor.file_to(store, outcomes=outcomes)
        legs[leg] = dict(actor=actor, store=store, on_games=on_games, rates=[], games=0, plies=0, pipelined=pipelined,
                         outcomes=outcomes, reported=0)
    dev = next(iter(legs.values()))["actor"].device

    def run(state, seconds):
        actor = state["actor"]
        torch.cuda.synchronize(dev)
        games0, plies0, t0 = actor.games_finished, actor.moves_played, time.perf_counter()
        while True:
            if state["pipelined"]:
                # the next batch of every group is queued before this one's games are filed; the window's last call
                # leaves nothing queued behind it, so every move the window counts was played inside it
                last = time.perf_counter() - t0 >= seconds
                actor.play_moves(M, 1.0, on_games=state["on_games"], prefetch=not last)
                if last:
                    break
                continue
            actor.play_moves(M, 1.0, on_games=state["on_games"])
            if state["outcomes"]:
                state["reported"] += len(actor.take_outcomes())
            if time.perf_counter() - t0 >= seconds:
                break
        actor.flush(on_games=state["on_games"])
        if state["outcomes"]:
            state["reported"] += len(actor.take_outcomes())
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - t0
        return actor.moves_played - plies0, actor.games_finished - games0, elapsed

    for state in legs.values():                       # warm-up: allocations, graph capture, the pre-drawn pipeline
        run(state, 0.0)
        run(state, 0.0)
    for _ in range(args.rounds):
        for state in legs.values():
            plies, games, elapsed = run(state, args.seconds)
            state["rates"].append(plies / elapsed)
            state["games"] += games
            state["plies"] += plies
    lines = []
    for leg, state in legs.items():
        rates = state["rates"]
        row = dict(config=args.config, leg=leg, groups=args.groups if state["pipelined"] else 1, envs=E, moves_per_batch=M, rounds=args.rounds, seconds_per_round=args.seconds,
                   moves_per_s=[round(r) for r in rates], median_moves_per_s=round(statistics.median(rates)),
                   spread=round((max(rates) - min(rates)) / statistics.median(rates), 4),
                   games=state["games"], mean_game_length=round(state["plies"] / max(1, state["games"]), 2),
                   measured="host clock closed by a device synchronise, legs alternated in one process")
        if state["outcomes"]:
            row["outcomes_reported"] = state["reported"]     # (warm-up batches included)
        if leg.split("_")[-1] == "device" or state["outcomes"]:
            row["filing_bytes_per_env_move"] = round(filing_bytes(config, E, M, state["games"], state["plies"]) / max(1, state["plies"]), 1)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        state["actor"].close()
        if state["store"] is not None:
            state["store"].close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
