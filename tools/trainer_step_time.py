#!/usr/bin/env python3
"""Time of Trainer.update_weights on the MI355X with the loss as one HIP launch (csrc/trainer_kernels.hip) and as the
torch expression: CartPole FC config and TicTacToe residual network, synthetic replay batches resident on the GPU.
One JSON line per (config, loss path).

--native-epilogue times the residual configs of --games (default tictactoe,connect4) instead, each eager and as a hipGraph,
each without and with Trainer(native_epilogue=True) (relu(batch_norm(x) [+ residual]) in training as one HIP launch each
way, csrc/bn_epilogue.hip): the ways are alternated, the unflagged first, --windows windows of at least --seconds each,
every window closed by a synchronise; one JSON line per (config, way) with the windows, their median and max - min, and for
the flagged ways whether a window overlaps one of the unflagged way of the same form.  --one-step WAY runs --steps steps of
one way and nothing else (for a kernel trace of that way alone: two traces with different --steps differ by whole steps).
--kernel-alone times the two launches at --shape (default Gomoku's layer, 512,128,11,11) against torch's expression.

--native-conv is the same protocol over four ways per form -- library, native_conv (the 3 x 3 convolutions and both gradients
as HIP launches, csrc/conv_train.hip), native_epilogue, both -- eager and as a hipGraph, all alternated in one process with
the unflagged way first; --one-step takes the names of these ways too.

--native-heads is that protocol over library, native_heads (the reward, value and policy heads as HIP launches,
csrc/head_train.hip), native_conv + native_epilogue, and all three flags; a line of the last way also says whether its windows
overlap those of native_conv + native_epilogue of the same form.  --one-step takes these names as well.

--native-rescale is that protocol over library, native_rescale (the backward of the hidden state's min-max rescale as one HIP
launch, csrc/rescale_train.hip, under the inference launch as the forward), the three earlier flags, and all four; a line of
the last way also says whether its windows overlap those of the three earlier flags.  --one-step takes these names too.

--native-optimizer is that protocol over two ways per form: the four flags with torch's optimizer ("four flags", the unflagged
way here, first) and the same with Trainer(native_optimizer=True) (the weight gradients folded and Adam applied in one HIP
launch, csrc/grad_fold.hip); a line of the second way says whether its windows overlap those of the first.  --one-step takes
these names too."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
pkg = lambda m: importlib.import_module("muzero-hypermodel_amd." + m)


def synthetic(config):
    model = pkg("models").MuZeroNetwork(config)
    ckpt = {"weights": model.get_weights(), "training_step": 0, "optimizer_state": None}
    B, K1, A = config.batch_size, config.num_unroll_steps + 1, len(config.action_space)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = (torch.rand((B,) + tuple(config.observation_shape), generator=g, device="cuda"),
             torch.randint(0, A, (B, K1), generator=g, device="cuda"),
             torch.randn(B, K1, generator=g, device="cuda") * 10, torch.randn(B, K1, generator=g, device="cuda"),
             torch.softmax(torch.randn(B, K1, A, generator=g, device="cuda"), dim=2),
             torch.rand(B, generator=g, device="cuda") + 0.5,
             torch.randint(1, K1 + 1, (B, K1), generator=g, device="cuda").float())
    return ckpt, batch, B, K1


def loss_paths():
    for game in ("cartpole", "tictactoe"):
        config = pkg("games." + game).MuZeroConfig()
        config.train_on_gpu = True
        ckpt, batch, B, K1 = synthetic(config)
        for native, graph in ((True, True), (True, False), (False, False)):
            trainer = pkg("trainer").Trainer(ckpt, config, device="cuda", graph=graph)
            trainer.native_loss = native
            for _ in range(10):
                trainer.update_weights(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 100
            for _ in range(n):
                trainer.update_weights(batch)
            torch.cuda.synchronize()
            print(json.dumps({"config": game, "batch": B, "unrolled_positions": K1, "loss": "one HIP launch" if native else "torch expression", "hipgraph": graph,
                              "ms_per_training_step": round((time.perf_counter() - t0) / n * 1e3, 3)}), flush=True)


def window(trainer, batch, seconds):
    """Steps until `seconds` have passed, in blocks of 10, closed by a synchronise: ms per step."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        for _ in range(10):
            trainer.update_weights(batch)
        n += 10
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if elapsed >= seconds:
            return elapsed / n * 1e3


WAYS = [("library, eager", dict(graph=False)), ("native_epilogue, eager", dict(graph=False, native_epilogue=True)),
        ("library, hipgraph", dict(graph=True)), ("native_epilogue, hipgraph", dict(graph=True, native_epilogue=True))]
FLAGS = [("library", {}), ("native_conv", dict(native_conv=True)), ("native_epilogue", dict(native_epilogue=True)),
         ("native_conv + native_epilogue", dict(native_conv=True, native_epilogue=True))]
CONV_WAYS = [(f"{name}, {form}", dict(graph=graph, **flags)) for form, graph in (("eager", False), ("hipgraph", True))
             for name, flags in FLAGS]
HEADS_FLAGS = [FLAGS[0], ("native_heads", dict(native_heads=True)), FLAGS[3],
               ("native_conv + native_epilogue + native_heads", dict(native_conv=True, native_epilogue=True, native_heads=True))]
HEADS_WAYS = [(f"{name}, {form}", dict(graph=graph, **flags)) for form, graph in (("eager", False), ("hipgraph", True))
              for name, flags in HEADS_FLAGS]
RESCALE_FLAGS = [FLAGS[0], ("native_rescale", dict(native_rescale=True)), HEADS_FLAGS[3],
                 ("native_conv + native_epilogue + native_heads + native_rescale",
                  dict(native_conv=True, native_epilogue=True, native_heads=True, native_rescale=True))]
RESCALE_WAYS = [(f"{name}, {form}", dict(graph=graph, **flags)) for form, graph in (("eager", False), ("hipgraph", True))
                for name, flags in RESCALE_FLAGS]
OPTIMIZER_FLAGS = [("four flags", RESCALE_FLAGS[3][1]), ("four flags + native_optimizer", dict(native_optimizer=True, **RESCALE_FLAGS[3][1]))]
OPTIMIZER_WAYS = [(f"{name}, {form}", dict(graph=graph, **flags)) for form, graph in (("eager", False), ("hipgraph", True))
                  for name, flags in OPTIMIZER_FLAGS]
ONE_STEP_WAYS = dict(CONV_WAYS + HEADS_WAYS + RESCALE_WAYS + OPTIMIZER_WAYS)
# the way whose windows a line of the all-flags way is also compared with: {prefix of the way: (prefix of the other, key)}
COMPARED = {"four flags + native_optimizer, ": ("four flags, ", "windows_overlap_four_flags"),
            "native_conv + native_epilogue + native_heads + native_rescale, ":
            ("native_conv + native_epilogue + native_heads, ", "windows_overlap_three_flags"),
            "native_conv + native_epilogue + native_heads, ": ("native_conv + native_epilogue, ", "windows_overlap_conv_and_epilogue")}


def epilogue_ways(args, ways=WAYS):
    for game in args.games.split(","):
        config = pkg("games." + game).MuZeroConfig()
        config.train_on_gpu = True
        torch.manual_seed(0)
        ckpt, batch, B, K1 = synthetic(config)
        if args.one_step is not None:
            trainer = pkg("trainer").Trainer(ckpt, config, device="cuda", **ONE_STEP_WAYS[args.one_step])
            for _ in range(args.steps):
                trainer.update_weights(batch)
            torch.cuda.synchronize()
            print(json.dumps({"config": game, "way": args.one_step, "steps": args.steps}), flush=True)
            continue
        trainers = []
        for name, how in ways:
            trainer = pkg("trainer").Trainer(ckpt, config, device="cuda", **how)
            for _ in range(5):
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
            if not name.startswith("library") and "library, " + name.rsplit(", ", 1)[1] in spans:
                lo, hi = spans["library, " + name.rsplit(", ", 1)[1]]
                line["windows_overlap_library"] = not (max(times) < lo or min(times) > hi)
            for prefix, (other, key) in COMPARED.items():
                if name.startswith(prefix) and other + name.rsplit(", ", 1)[1] in spans:
                    lo, hi = spans[other + name.rsplit(", ", 1)[1]]
                    line[key] = not (max(times) < lo or min(times) > hi)
            print(json.dumps(line), flush=True)


def kernel_alone(args):
    """Forward + backward of the epilogue at one shape, with a residual: the two HIP launches against torch's expression,
    both through autograd; the bytes the shape needs are x, residual and dy read once, out, dx and dresidual written once."""
    models = pkg("models")
    shape = tuple(int(v) for v in args.shape.split(","))
    n, c, h, w = shape
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(shape, generator=g, device="cuda").requires_grad_()
    residual = torch.randn(shape, generator=g, device="cuda").requires_grad_()
    dy = torch.randn(shape, generator=g, device="cuda")
    needed = 6 * x.numel() * 4
    times = {}
    for name, on in (("torch expression", False), ("native_epilogue", True)) * args.windows:
        bn = models.BatchNorm2d(c).cuda().train()
        bn.native_training = on

        def once():
            x.grad = residual.grad = None
            models.conv_epilogue(x, bn, residual).backward(dy)

        for _ in range(5):
            once()
        torch.cuda.synchronize()
        t0, count = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.seconds:
            for _ in range(20):
                once()
            count += 20
            torch.cuda.synchronize()
        times.setdefault(name, []).append((time.perf_counter() - t0) / count * 1e3)
    for name, values in times.items():
        median = statistics.median(values)
        print(json.dumps({"shape": list(shape), "way": name, "forward_plus_backward_ms_windows": [round(v, 4) for v in values],
                          "median_ms": round(median, 4), "max_minus_min_ms": round(max(values) - min(values), 4),
                          "bytes_needed": needed, "achieved_GB_per_s": round(needed / (median * 1e-3) / 1e9, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--native-epilogue", action="store_true")
    ap.add_argument("--native-conv", action="store_true")
    ap.add_argument("--native-heads", action="store_true")
    ap.add_argument("--native-rescale", action="store_true")
    ap.add_argument("--native-optimizer", action="store_true")
    ap.add_argument("--kernel-alone", action="store_true")
    ap.add_argument("--one-step", default=None, metavar="WAY", help="one of: " + "; ".join(ONE_STEP_WAYS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--games", default="tictactoe,connect4")
    ap.add_argument("--shape", default="512,128,11,11")
    args = ap.parse_args()
    if args.kernel_alone:
        kernel_alone(args)
    elif args.native_conv:
        epilogue_ways(args, CONV_WAYS)
    elif args.native_heads:
        epilogue_ways(args, HEADS_WAYS)
    elif args.native_rescale:
        epilogue_ways(args, RESCALE_WAYS)
    elif args.native_optimizer:
        epilogue_ways(args, OPTIMIZER_WAYS)
    elif args.native_epilogue or args.one_step is not None:
        epilogue_ways(args)
    else:
        loss_paths()


if __name__ == "__main__":
    main()
