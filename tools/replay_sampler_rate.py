#!/usr/bin/env python3
"""The replay store's device sampler against host sampling (ReplayBuffer(device_sampling=...)), one MI355X:

* the sampler launch alone (mzreplay_sample_batch: four kernels), HIP events over --launches launches after warm-up;
* get_batch() per second in both modes (the device mode's calls are queued and waited for once at the end);
* with --train: whole training steps per second in both modes (host: get_batch -> update_lr -> update_weights ->
  update_priorities; device: Trainer.train_steps), Trainer(graph=True) where the network allows it.

    python tools/replay_sampler_rate.py --shape cartpole|tictactoe|connect4|gomoku [--games N] [--train] [--sampler-only]

Games are synthetic (random lengths up to max_moves, random priorities through the store's own kernel); shapes, batch and
unroll sizes are the game's config.  One JSON line.  For the split between the four kernels run the --sampler-only form
under `rocprofv3 --kernel-trace --stats` (sample_walk_kernel is the serial walk)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
DEFAULT_GAMES = {"cartpole": 500, "tictactoe": 3000, "connect4": 10000, "gomoku": 2000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cartpole", choices=sorted(DEFAULT_GAMES))
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--sampler-only", action="store_true")
    args = ap.parse_args()
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{args.shape}").MuZeroConfig()
    G = args.games or DEFAULT_GAMES[args.shape]
    config.replay_buffer_size = G
    A, L = len(config.action_space), int(config.max_moves)
    rs = np.random.RandomState(5)
    low = max(1, L // 8)
    lengths = rs.randint(low, L + 1, G).astype(np.int32)
    shape = tuple(int(v) for v in config.observation_shape)
    players = len(config.players)
    packed = sp.PackedGames(
        env_index=np.arange(G), length=lengths,
        observations=rs.random_sample((G, L + 1) + shape).astype(np.float32),
        actions=rs.randint(0, A, (G, L + 1)).astype(np.int32), rewards=rs.standard_normal((G, L + 1)),
        to_play=(np.arange(L + 1)[None, :] % players).repeat(G, axis=0).astype(np.int32),
        child_visits=rs.dirichlet([0.6] * A, (G, L)), root_values=rs.standard_normal((G, L)) * 3)
    out = {"shape": args.shape, "games": G, "batch_size": int(config.batch_size), "unroll_plus_1": config.num_unroll_steps + 1,
           "max_moves": L, "actions": A, "PER": bool(config.PER)}

    dev = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config, device_sampling=True)
    dev.save_games(packed)
    for _ in range(10):
        dev.get_batch()
    torch.cuda.synchronize()
    # the sampler launch alone
    import ctypes
    B, U1 = int(config.batch_size), config.num_unroll_steps + 1
    ids = torch.empty(B, dtype=torch.int64, device="cuda")
    slots, pos = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    absorbing = torch.empty((B, U1), dtype=torch.int32, device="cuda")
    weights = torch.empty(B, dtype=torch.float32, device="cuda")

    def sample():
        dev._check(dev._lib.mzreplay_sample_batch(dev._h, B, 0, G, int(dev.total_samples), 1 if config.PER else 0,
                                                  ids.data_ptr(), slots.data_ptr(), pos.data_ptr(), absorbing.data_ptr(),
                                                  weights.data_ptr(), dev._stream()))
    for _ in range(10):
        sample()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.launches):
        sample()
    stop.record()
    torch.cuda.synchronize()
    out["sampler_launch_us"] = 1e3 * start.elapsed_time(stop) / args.launches
    out["sampler_launches_timed"] = args.launches
    if not args.sampler_only:
        t0 = time.perf_counter()
        for _ in range(args.launches):
            dev.get_batch()
        torch.cuda.synchronize()
        out["get_batch_per_s_device_sampling"] = args.launches / (time.perf_counter() - t0)
        host = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)
        host.save_games(packed)
        for _ in range(3):
            host.get_batch()
        torch.cuda.synchronize()
        reps = max(10, args.launches // 10)
        t0 = time.perf_counter()
        for _ in range(reps):
            host.get_batch()
        torch.cuda.synchronize()
        out["get_batch_per_s_host_sampling"] = reps / (time.perf_counter() - t0)
        if args.train:
            tr_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
            models = importlib.import_module("muzero-hypermodel_amd.models")
            torch.manual_seed(0)
            weights0 = models.MuZeroNetwork(config).get_weights()
            graph = config.network == "fullyconnected"
            out["trainer_graph"] = graph
            for mode, rb in (("host", host), ("device", dev)):
                trainer = tr_mod.Trainer({"weights": weights0, "training_step": 0, "optimizer_state": None}, config,
                                         device="cuda", graph=graph)

                def steps(n):
                    if mode == "device":
                        trainer.train_steps(rb, n)
                        return
                    for _ in range(n):
                        index_batch, batch = rb.get_batch()
                        trainer.update_lr()
                        priorities, *_ = trainer.update_weights(batch)
                        if config.PER:
                            rb.update_priorities(priorities, index_batch)
                steps(10)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps(args.train_steps)
                torch.cuda.synchronize()
                out[f"train_steps_per_s_{mode}_sampling"] = args.train_steps / (time.perf_counter() - t0)
        host.close()
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
