#!/usr/bin/env python3
"""BASELINE.json config #4 as one command: N self-play actors, one per GPU, device-resident envs, the reference's
continuous_self_play loop on every actor (self_play.ManyEnvLoop), fresh weights from rank 0's shared storage to all
actors by ONE RCCL broadcast of the flat buffer every `--moves-per-pass` moves (muzero.py:170-186 without Ray).

    python tools/selfplay_actors.py --gpus 8 --game connect4 --envs 1024 --passes 20 --moves-per-pass 4

Starts its ranks itself (like bench.py) or joins the group torch.distributed.run made.  The "trainer" here is a stand-in
that bumps the training step and perturbs the weights after every pass (there is no replay-driven training in this
tool): what is exercised is the actor side -- search, envs, history filing, the weight pull and its version stamps.
Prints one JSON line (rank 0): games, moves and simulations per second over all ranks.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


def pkg(sub):
    return importlib.import_module(f"muzero-hypermodel_amd.{sub}")


class Storage:
    """Rank 0's shared_storage stand-in (shared_storage.py:1-39): info dict + a trainer that publishes after each pass."""

    def __init__(self, weights, training_steps):
        self.info = {"training_step": 0, "terminate": False, "weights": weights, "num_played_steps": 0,
                     "num_played_games": 0}
        self.training_steps = training_steps

    def get_info(self, key):
        return self.info[key]

    def set_info(self, keys, values=None):
        self.info.update(keys)

    def trainer_step(self):
        self.info["training_step"] += 1
        self.info["weights"] = {k: (v * 0.999 if v.dtype == torch.float32 else v) for k, v in self.info["weights"].items()}


class Replay:
    def __init__(self, storage):
        self.storage, self.games, self.moves, self.versions = storage, 0, 0, set()

    def save_game(self, game_history, shared_storage=None):
        self.games += 1
        self.moves += len(game_history.action_history) - 1
        self.versions.add(game_history.weights_version)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--game", choices=["connect4", "tictactoe", "gomoku", "cartpole"], default="connect4")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--moves-per-pass", type=int, default=4)
    ap.add_argument("--groups", type=int, default=1,
                    help="board games: engine groups per actor on streams of their own (PipelinedDeviceSelfPlay: pays from tens of thousands of envs per GPU on); 1 = one engine")
    ap.add_argument("--temperature", type=float, default=None,
                    help="softmax temperature of every pass (default: the config's visit_softmax_temperature_fn)")
    ap.add_argument("--device-temperatures", action="store_true",
                    help="passes at a temperature other than 0 and 1 / k, k = 1..4, run as move batches too: sampled on the GPU "
                         "(set_device_temperatures); without it they go move by move")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        bench = importlib.import_module("bench")
        launch_args = argparse.Namespace(gpus=args.gpus, rehearse_cpu=False)
        old = bench.__file__
        bench.__file__ = os.path.abspath(__file__)            # the ranks are copies of THIS script
        try:
            sys.exit(bench.launch_ranks(launch_args, sys.argv[1:]))
        finally:
            bench.__file__ = old
    actor_mod, sp = pkg("actor"), pkg("self_play")
    rank, world, local_rank = actor_mod.init_distributed()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    config = pkg(f"games.{args.game}").MuZeroConfig()
    config.training_steps, config.ratio, config.self_play_delay = args.passes, None, 0
    if args.temperature is not None:
        config.visit_softmax_temperature_fn = lambda trained_steps: args.temperature
    if args.game == "cartpole":
        from parity_helpers import load_golden
        w = load_golden("cartpole_weights")
        weights = {k: torch.from_numpy(w[k]) for k in w.files}
    else:
        from synth import synthetic_state_dict
        template = pkg("models").MuZeroNetwork(config).state_dict()
        weights = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(template, 0).items()}
    storage = Storage(weights, args.passes) if rank == 0 else None
    replay = Replay(storage)
    if args.groups > 1 and config.network != "fullyconnected":
        actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, args.game, config, config.seed + rank * args.envs, args.envs,
                                           groups=args.groups, device=device)
    else:
        actor = sp.DeviceSelfPlay({"weights": weights}, args.game, config, config.seed + rank * args.envs, args.envs, device=device)

    if args.device_temperatures:
        actor.set_device_temperatures(True)

    play_pass = actor._play_pass

    def pass_then_train(temperature, threshold, moves_per_pass):   # the stand-in trainer publishes after every pass
        finished = play_pass(temperature, threshold, moves_per_pass)
        if storage is not None:
            storage.trainer_step()
        return finished
    actor._play_pass = pass_then_train
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    actor.continuous_self_play(storage, replay, False, moves_per_pass=args.moves_per_pass)
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0
    stats = [replay.games, replay.moves, actor.moves_played, elapsed, sorted(replay.versions)[-3:]]
    if world > 1:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, stats)
    else:
        gathered = [stats]
    if rank == 0:
        moves = sum(g[2] for g in gathered)
        wall = max(g[3] for g in gathered)
        print(json.dumps({"game": args.game, "actors": world, "envs_per_actor": args.envs, "passes": args.passes,
                          "moves_per_pass": args.moves_per_pass, "games_finished": sum(g[0] for g in gathered),
                          "moves_played": moves, "moves_per_s": moves / wall,
                          "simulations_per_s": moves * config.num_simulations / wall,
                          "weight_versions_seen_last": gathered[0][4],
                          "collective_backend": torch.distributed.get_backend() if world > 1 else None}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
