#!/usr/bin/env python3
"""Time of one training step of a fully-connected network on the MI355X: today's graphed step (torch forward and backward,
the loss as one HIP launch, replayed as a hipGraph) against Trainer(fc_step=True) (forward, loss, backward and weight
gradients as four HIP launches), eager and graphed.  CartPole and SimpleGrid configs at their own batch sizes, synthetic
replay batches resident on the GPU.  The ways are alternated, today's first, `--windows` windows of at least `--seconds`
each, every window closed by a synchronise; one JSON line per (config, way) with the windows, their median and max - min.
Without --fc-step only today's way is timed.  --fc-optimizer (implies --fc-step) appends Trainer(fc_step=True,
fc_optimizer=True), the optimizer as a HIP launch on the flat buffers, eager and graphed, to the same alternation; its lines
also say whether their windows overlap those of the fc_step way of the same form.  --one-step WAY runs --steps steps of one
way and nothing else (for a kernel trace of that way alone: two traces with different --steps differ by whole steps)."""
import argparse, importlib, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
pkg = lambda m: importlib.import_module("muzero-hypermodel_amd." + m)


def window(trainer, batch, seconds):
    """Steps until `seconds` have passed, in blocks of 50, closed by a synchronise: ms per step."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        for _ in range(50):
            trainer.update_weights(batch)
        n += 50
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if elapsed >= seconds:
            return elapsed / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fc-step", action="store_true", help="also time Trainer(fc_step=True), eager and graphed")
    ap.add_argument("--fc-optimizer", action="store_true",
                    help="also time Trainer(fc_step=True, fc_optimizer=True), eager and graphed (implies --fc-step)")
    ap.add_argument("--one-step", default=None, metavar="WAY",
                    help="run --steps steps of this way alone (\"library, eager\" is a way here too) and print a marker line")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--games", default="cartpole,simple_grid")
    args = ap.parse_args()
    args.fc_step = args.fc_step or args.fc_optimizer
    for game in args.games.split(","):
        config = pkg("games." + game).MuZeroConfig()
        config.train_on_gpu = True
        torch.manual_seed(0)
        model = pkg("models").MuZeroNetwork(config)
        ckpt = {"weights": model.get_weights(), "training_step": 0, "optimizer_state": None}
        B, K1, A = config.batch_size, config.num_unroll_steps + 1, len(config.action_space)
        c, h, w = config.observation_shape
        stacked = (c * (config.stacked_observations + 1) + config.stacked_observations, h, w)
        g = torch.Generator(device="cuda").manual_seed(0)
        batch = (torch.rand((B,) + stacked, generator=g, device="cuda"),
                 torch.randint(0, A, (B, K1), generator=g, device="cuda"),
                 torch.randn(B, K1, generator=g, device="cuda") * 10, torch.randn(B, K1, generator=g, device="cuda"),
                 torch.softmax(torch.randn(B, K1, A, generator=g, device="cuda"), dim=2),
                 torch.rand(B, generator=g, device="cuda") + 0.5,
                 torch.randint(1, K1 + 1, (B, K1), generator=g, device="cuda").float())
        ways = [("library, hipgraph", dict(graph=True))]
        if args.fc_step:
            ways += [("fc_step, eager", dict(graph=False, fc_step=True)), ("fc_step, hipgraph", dict(graph=True, fc_step=True))]
        if args.fc_optimizer:
            ways += [("fc_step + fc_optimizer, eager", dict(graph=False, fc_step=True, fc_optimizer=True)),
                     ("fc_step + fc_optimizer, hipgraph", dict(graph=True, fc_step=True, fc_optimizer=True))]
        if args.one_step is not None:
            ways = [("library, eager", dict(graph=False))] + ways
            how = dict(ways)[args.one_step]
            trainer = pkg("trainer").Trainer(ckpt, config, device="cuda", **how)
            for _ in range(args.steps):
                trainer.update_weights(batch)
            torch.cuda.synchronize()
            print(json.dumps({"config": game, "way": args.one_step, "steps": args.steps}), flush=True)
            continue
        trainers = []
        for name, how in ways:
            trainer = pkg("trainer").Trainer(ckpt, config, device="cuda", **how)
            for _ in range(10):
                trainer.update_weights(batch)
            trainers.append((name, trainer, []))
        for _ in range(args.windows):
            for name, trainer, times in trainers:
                times.append(window(trainer, batch, args.seconds))
        spans = {name: (min(times), max(times)) for name, trainer, times in trainers}
        for name, trainer, times in trainers:
            line = {"config": game, "batch": B, "unrolled_positions": K1, "way": name,
                    "ms_per_training_step_windows": [round(t, 4) for t in times],
                    "median_ms": round(statistics.median(times), 4), "max_minus_min_ms": round(max(times) - min(times), 4)}
            if name.startswith("fc_step + fc_optimizer"):
                lo, hi = spans[name.replace(" + fc_optimizer", "")]
                line["windows_overlap_fc_step"] = not (max(times) < lo or min(times) > hi)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
