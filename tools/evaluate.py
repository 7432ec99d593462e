"""Evaluation games on device-resident envs: MuZero against the expert / a random player / itself.

    python tools/evaluate.py --game tictactoe --envs 65536 --tests 200000 [--opponent expert] [--muzero-player 0]
                             [--fc 0] [--batch 8] [--groups 1] [--warmup-batches 3] [--compare-self] [--max-moves N]
                             [--temperature 0.35 --device-temperatures] [--paired]

Prints one JSON line: self_play.evaluate's result (MuZero.test's number, rewards per side, win / draw / loss counts, mean
episode length) with games per second, env-moves per second, simulations per second, the share of plies the opponent
played and the share of env-moves that sat a search out (searched plies are counted by the history filer, not estimated).  The warm-up batches run on the actor
that is timed afterwards (buffers, hipGraph capture and filer are set up in them); a rate is worth quoting when
`seconds` is at least one -- raise --tests otherwise.  --compare-self adds the same command line played as "self"
(every ply searched) for the ratio.  --paired: the opponent replies inside MuZero's move, so no env sits a search out
(the same games); with --compare-self the sit-out mode of the same command line is added as "sit_out" beside "self".
Weights are the seed-0 initialisation unless --weights points to a checkpoint (torch.save of {"weights": ...})."""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

sp = importlib.import_module("muzero-hypermodel_amd.self_play")
models = importlib.import_module("muzero-hypermodel_amd.models")


def run(args, config, checkpoint, opponent, num_tests, paired=False):
    out = sp.evaluate(checkpoint, args.game, config, num_tests, opponent=opponent, muzero_player=args.muzero_player,
                      num_envs=args.envs, seed=args.seed, moves_per_batch=args.batch, groups=args.groups,
                      warmup_batches=args.warmup_batches, temperature=args.temperature,
                      device_temperatures=args.device_temperatures, paired=paired)
    s = out["seconds"]
    out.update(games_per_s=out["games"] / s, env_moves_per_s=out["env_moves"] / s, simulations_per_s=out["simulations"] / s,
               opponent_ply_share=1.0 - out["searched_moves"] / max(1, out["env_moves"]))
    # (sit-out mode: an opponent's ply is an env that sat a search out; paired mode: no env sits a search out)
    out["sat_out_share"] = 0.0 if out.get("paired") else out["opponent_ply_share"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="tictactoe", choices=["tictactoe", "connect4", "gomoku", "cartpole", "twentyone", "simple_grid"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--tests", type=int, default=20000, help="games to average (the first N started)")
    ap.add_argument("--opponent", default=None, choices=["self", "expert", "random"], help="default: the config's")
    ap.add_argument("--muzero-player", type=int, default=None, help="default: the config's")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8, help="moves per host round trip")
    ap.add_argument("--groups", type=int, default=1, help="> 1: env groups on HIP streams of their own")
    ap.add_argument("--fc", type=int, default=0, help="N > 0: a fully-connected network of N units (fused whole-move search)")
    ap.add_argument("--weights", default=None, help="checkpoint file; default: seed-0 initialisation")
    ap.add_argument("--warmup-batches", type=int, default=3, help="untimed batches on the same actor first (code objects, "
                    "rings, graph capture, filer); games that begin in them are not counted")
    ap.add_argument("--compare-self", action="store_true")
    ap.add_argument("--temperature", type=float, default=0.0, help="softmax temperature of MuZero's moves (MuZero.test: 0)")
    ap.add_argument("--device-temperatures", action="store_true", help="a temperature other than 0, inf and 1 / k, k = 1..4, "
                    "sampled on the GPU: batches (and plies against an opponent at all) instead of one move per round trip")
    ap.add_argument("--paired", action="store_true", help="the opponent replies inside MuZero's move: every env is searched "
                    "in every move (evaluate(paired=True))")
    ap.add_argument("--max-moves", type=int, default=None, help="end games after N plies (config.max_moves; default: the "
                    "config's)")
    args = ap.parse_args()
    mod = importlib.import_module(f"muzero-hypermodel_amd.games.{args.game}")
    config = mod.MuZeroConfig()
    if args.max_moves is not None:
        config.max_moves = args.max_moves
    if args.fc:
        config.network, config.encoding_size = "fullyconnected", args.fc
        config.fc_representation_layers, config.fc_dynamics_layers = [], [args.fc]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [args.fc]
    if args.weights:
        checkpoint = torch.load(args.weights, map_location="cpu")
    else:
        torch.manual_seed(0)
        checkpoint = {"weights": models.MuZeroNetwork(config).get_weights()}
    opponent = args.opponent if args.opponent is not None else config.opponent
    line = run(args, config, checkpoint, opponent, args.tests, paired=args.paired)
    line.update(game=args.game, network=config.network, max_moves=config.max_moves)
    if args.compare_self and opponent != "self":
        line["self"] = run(args, config, checkpoint, "self", args.tests)
        line["simulations_vs_self"] = line["simulations_per_s"] / line["self"]["simulations_per_s"]
        if args.paired:
            line["sit_out"] = run(args, config, checkpoint, opponent, args.tests)
            line["games_vs_sit_out"] = line["games_per_s"] / line["sit_out"]["games_per_s"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
