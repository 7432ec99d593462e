#!/usr/bin/env python3
"""The closed training loop on one MI355X for any device game (muzero-hypermodel_amd/training_loop.py TrainingLoop):
device self-play in move batches -> games filed into the replay store on the device, with their outcomes -> replay batches
drawn on the device -> Trainer.train_steps -> optional batched Reanalyse -> weights published -> optional evaluation.

    python tools/train.py --game cartpole|tictactoe|connect4|gomoku|twentyone|simple_grid [--envs 64] [--iterations 30]
                          [--moves 8] [--train-steps 100] [--seed 0] [--reanalyse N] [--eval-every K --eval-games G]
                          [--eval-opponent expert|random|self] [--eval-paired] [--groups N] [--host-filing] [--seconds S]
                          [--set key=value ...] [--log PATH]

--set key=value overrides an attribute of the game's MuZeroConfig (the value is a Python literal: --set num_simulations=10
--set batch_size=16 --set "fc_value_layers=[16]"), so that small runs are possible.
--seconds S ends the run after the first iteration that finishes past S seconds of wall time (a bounded run).
--log PATH writes the rows as JSON lines to PATH as well as to standard output.
With --game cartpole and no other option the sizes are tools/train_cartpole.py's, and mean_total_reward is its
mean_reward_last_50, row for row, at the same seed (CartPole pays 1 per move)."""
import argparse
import ast
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    loop_mod = importlib.import_module("muzero-hypermodel_amd.training_loop")
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", required=True, choices=loop_mod.DEVICE_GAMES)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--moves", type=int, default=8, help="self-play moves per env and iteration (one move batch)")
    ap.add_argument("--train-steps", type=int, default=100, help="training steps per iteration")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reanalyse", type=int, default=0, help="games per iteration refreshed by a batched Reanalyse pass")
    ap.add_argument("--eval-every", type=int, default=0, help="evaluate every K iterations (0: never)")
    ap.add_argument("--eval-games", type=int, default=0)
    ap.add_argument("--eval-opponent", default=None, choices=["self", "expert", "random"], help="default: the config's")
    ap.add_argument("--eval-paired", action="store_true", help="evaluation games: the opponent replies inside MuZero's move "
                    "(the same games; no env sits a search out)")
    ap.add_argument("--groups", type=int, default=1, help="> 1: env groups on HIP streams of their own")
    ap.add_argument("--host-filing", action="store_true", help="games through on_games -> save_games (the twin of the default)")
    ap.add_argument("--seconds", type=float, default=None, help="stop after the iteration that ends past this wall time")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="override a MuZeroConfig attribute")
    ap.add_argument("--log", default=None, help="also write the rows to this file (JSON lines)")
    args = ap.parse_args()
    overrides = {}
    for item in args.set:
        key, sep, text = item.partition("=")
        if not sep:
            ap.error(f"--set wants key=value, not {item!r}")
        try:
            overrides[key] = ast.literal_eval(text)
        except (ValueError, SyntaxError):
            overrides[key] = text                      # a bare word: a string
    config = loop_mod.game_config(args.game, overrides)
    if "training_steps" not in overrides:
        config.training_steps = args.iterations * args.train_steps    # (the temperature and lr schedules span the run)
    out = open(args.log, "w") if args.log else None

    def say(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    loop = loop_mod.TrainingLoop(args.game, config, args.envs, args.moves, args.train_steps, args.seed,
                                 reanalyse_games=args.reanalyse, eval_every=args.eval_every, eval_games=args.eval_games,
                                 eval_opponent=args.eval_opponent, groups=args.groups, device_filing=not args.host_filing,
                                 log=lambda text: say({"note": text}), eval_paired=args.eval_paired)
    for _ in range(args.iterations):
        row = loop.iterate()
        say(row)
        if args.seconds is not None and row["seconds"] >= args.seconds:
            break
    loop.close()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
