"""Whole self-play loop rate (search + env step + history filing), host-plugin envs vs device envs.

    python tools/selfplay_rate.py [--game cartpole] [--envs 4096] [--moves 60] [--max-moves N]
    python tools/selfplay_rate.py --game gomoku --kinds search,device-batch [--simulations S --channels C --blocks B]
    python tools/selfplay_rate.py --kinds device-batch --temperature 0.35 --device-temperatures
    python tools/selfplay_rate.py --game tictactoe --fc 16 --stacked 2 --kinds host,device-batch

Prints one JSON line per actor kind: moves/s, simulations/s, finished games, the engine's device bytes.  This is the
loop the reference runs in self_play.py:34-113 (continuous_self_play), without the replay buffer hand-off.  Kind
"search" times the search alone (fixed start positions, no env step, no filing) for comparison with the whole loop.

Gomoku at the reference's config (400 simulations, 6 blocks x 128 channels, 11 x 11) is heavy: a tree holds 401 hidden
states of 62 KB, about 26 MB per env, so its default is 256 envs (~7 GB); the towers run as PyTorch-ROCm convolutions
(there is no 11 x 11 tower kernel)."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

sp = importlib.import_module("muzero-hypermodel_amd.self_play")
models = importlib.import_module("muzero-hypermodel_amd.models")


def engine_bytes(actor):
    """Device bytes of the actor's search engine(s): trees, hidden-state pool, per-move buffers."""
    actors = getattr(actor, "actors", [actor])
    return int(sum(a.engine.device_bytes() for a in actors))


def search_only(args, config, weights):
    """The search alone: every env searches its start position `--moves` times (no env step, no history filing)."""
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    device_mod = importlib.import_module("muzero-hypermodel_amd.games.device")
    model = models.MuZeroNetwork(config)
    model.set_weights(weights)
    model.to("cuda").eval()
    envs = device_mod.DeviceEnvs(args.game, args.envs)
    obs, legal, num_legal, to_play = envs.observe()
    torch.cuda.synchronize()
    n = num_legal.cpu().tolist()
    legal_lists = [row[:k] for row, k in zip(legal.cpu().tolist(), n)]
    to_play = to_play.cpu().tolist()
    engine = engine_mod.BatchedMCTS(config, args.envs, device="cuda", use_graph=True)
    with torch.no_grad():
        for _ in range(2):
            engine.search(model, obs, legal_lists, to_play, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.moves):
            engine.search(model, obs, legal_lists, to_play, True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    moves = args.moves * args.envs
    print(json.dumps({"actor": "search", "game": args.game, "envs": args.envs, "moves_per_s": moves / dt,
                      "simulations_per_s": moves * config.num_simulations / dt, "ms_per_move_step": 1e3 * dt / args.moves,
                      "num_simulations": config.num_simulations, "engine_device_bytes": engine.device_bytes()}), flush=True)
    engine.close()
    envs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="cartpole",
                    choices=["cartpole", "tictactoe", "connect4", "gomoku", "twentyone", "simple_grid"])
    ap.add_argument("--envs", type=int, default=None, help="default 4096; gomoku 256 (a tree is ~26 MB at its config)")
    ap.add_argument("--moves", type=int, default=60)
    ap.add_argument("--kinds", default="host,device")
    ap.add_argument("--batch", type=int, default=20, help="moves per host round trip of the device-batch actor")
    ap.add_argument("--weights", default="random", choices=["random", "checkpoint"],
                    help="checkpoint: the reference's trained CartPole weights (tests/golden/cartpole_weights.npz): long "
                         "games and the benchmark's tree depths; random: seed-0 initialisation, games of ~15 moves")
    ap.add_argument("--fc", type=int, default=0, help="N > 0: play the game with a fully-connected network (the reference's "
                    "network = 'fullyconnected'), encoding and layers of N units -- board games through the fused whole-move search")
    ap.add_argument("--no-prefetch", action="store_true", help="device-pipelined-batch: every play_moves call drains the GPU "
                    "(what a loop does that pulls weights between calls)")
    ap.add_argument("--max-moves", type=int, default=None, help="end games after N plies (config.max_moves; default: the "
                    "config's): the device actors' batches apply it in the environment kernels")
    ap.add_argument("--simulations", type=int, default=None, help="config.num_simulations (default: the config's)")
    ap.add_argument("--channels", type=int, default=None, help="config.channels of a residual network (default: the config's)")
    ap.add_argument("--blocks", type=int, default=None, help="config.blocks of a residual network (default: the config's)")
    ap.add_argument("--temperature", type=float, default=1.0, help="softmax temperature of the action sampling")
    ap.add_argument("--device-temperatures", action="store_true", help="device actors: batches sample at any temperature on "
                    "the GPU (set_device_temperatures); without it the batch kinds take 0 and 1 / k, k = 1..4, only")
    ap.add_argument("--stacked", type=int, default=0, help="config.stacked_observations: the searches read the current frame "
                    "and the N previous ones (device actors: the frame stack on the GPU; random weights only)")
    args = ap.parse_args()
    if args.stacked and (args.weights == "checkpoint" or "search" in args.kinds.split(",")):
        ap.error("--stacked changes the network's input: random weights, and no search-only kind (it has no history to stack)")
    if args.envs is None:
        args.envs = 256 if args.game == "gomoku" else 4096
    mod = importlib.import_module(f"muzero-hypermodel_amd.games.{args.game}")
    config = mod.MuZeroConfig()
    for name, value in (("num_simulations", args.simulations), ("channels", args.channels), ("blocks", args.blocks)):
        if value is not None:
            setattr(config, name, value)
    if args.max_moves is not None:
        config.max_moves = args.max_moves
    config.stacked_observations = args.stacked
    if args.fc:
        config.network, config.encoding_size = "fullyconnected", args.fc
        config.fc_representation_layers, config.fc_dynamics_layers = [], [args.fc]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [args.fc]
        config.temperature_threshold = None
    torch.manual_seed(0)
    weights = models.MuZeroNetwork(config).get_weights()
    if args.weights == "checkpoint":
        import numpy
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        fixture = numpy.load(os.path.join(root, "tests", "golden", "cartpole_weights.npz"))
        weights = {k: torch.from_numpy(fixture[k]) for k in fixture.files}
    for kind in args.kinds.split(","):
        if kind == "search":
            search_only(args, config, weights)
            continue
        if kind == "host":
            actor = sp.BatchedSelfPlay({"weights": weights}, mod.Game, config, 0, args.envs)
        elif kind in ("device-pipelined", "device-pipelined-batch"):
            actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, args.game, config, 0, args.envs, groups=2)
        else:
            actor = sp.DeviceSelfPlay({"weights": weights}, args.game, config, 0, args.envs)
            if kind == "device-batch" and actor.engine._fc_model is not None:
                actor.engine.set_fused_options("auto", publish_tree=False)
        if args.device_temperatures and kind != "host":
            actor.set_device_temperatures(True)
        done = [0]

        def on_game(e, gh):
            done[0] += 1

        def on_games(batch):
            done[0] += len(batch)

        cb = dict(on_game=on_game) if kind in ("host", "device-lists") else dict(on_games=on_games)
        if kind in ("device-batch", "device-pipelined-batch"):
            # searches, env steps and resets queued back to back, `--batch` moves per host round trip
            for _ in range(3):                       # buffers, the native history filer, the pre-drawn next batch
                actor.play_moves(args.batch, args.temperature, **cb)
            torch.cuda.synchronize()
            done[0] = 0
            t0 = time.perf_counter()
            moves = 0
            calls = max(1, args.moves // args.batch)
            for i in range(calls):
                # (two groups: each group's next batch is queued before its last one is filed; the last call drains)
                ahead = dict(prefetch=i + 1 < calls and not args.no_prefetch) if kind == "device-pipelined-batch" else {}
                moves += int(actor.play_moves(args.batch, args.temperature, **cb, **ahead).sum())
            actor.flush(**cb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        else:
            for _ in range(5):
                actor.step(args.temperature, None, **cb)
            torch.cuda.synchronize()
            done[0] = 0
            t0 = time.perf_counter()
            for _ in range(args.moves):
                actor.step(args.temperature, None, **cb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            moves = args.moves * args.envs
        print(json.dumps({"actor": kind, "game": args.game, "envs": args.envs, "moves_per_s": moves / dt,
                          "simulations_per_s": moves * config.num_simulations / dt, "ms_per_move_step": 1e3 * dt * args.envs / moves,
                          "games_finished": done[0], "weights": args.weights, "max_moves": config.max_moves,
                          "num_simulations": config.num_simulations, "engine_device_bytes": engine_bytes(actor),
                          "stacked_observations": config.stacked_observations, "seconds": dt, "network": config.network,
                          "temperature": args.temperature, "device_temperatures": bool(args.device_temperatures and kind != "host"),
                          **({"moves_per_call": args.batch, "prefetch": not args.no_prefetch} if kind == "device-pipelined-batch" else {}),
                          **({"moves_per_call": args.batch} if kind == "device-batch" else {})}), flush=True)
        actor.close()


if __name__ == "__main__":
    main()
