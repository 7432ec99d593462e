"""Time of one Gomoku `advance` launch (step, observation, reset of finished envs, next observation) at E envs.

    python tools/gomoku_env_time.py [--envs 4096] [--launches 2000]
    MZENV_GOMOKU_SERIAL=1 python tools/gomoku_env_time.py        # the one-thread-per-env form of the same rules

Every launch plays a random legal cell in every env (chosen on the device from the kernel's own legal lists), so games
end by fives and restart all the time, as in self-play.  Prints one JSON line with the host-clock time per launch
(action choice included); the kernel's own time comes from running this under `rocprofv3 --kernel-trace --stats`
(kernel gomoku_env_kernel<3> / gomoku_env_serial_kernel<3>), each form in a process of its own."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    device = importlib.import_module("muzero-hypermodel_amd.games.device")
    E = args.envs
    envs = device.DeviceEnvs("gomoku", E)
    envs.observe()
    reward, done = torch.zeros(E, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
    obs_after, obs_next = torch.zeros((E, 3, 11, 11), device="cuda"), torch.zeros((E, 3, 11, 11), device="cuda")
    generator = torch.Generator(device="cuda").manual_seed(0)
    games = torch.zeros((), dtype=torch.int64, device="cuda")

    def advance():
        pick = (torch.rand(E, device="cuda", generator=generator) * envs.num_legal).long().clamp_(max=120)
        actions = envs.legal.gather(1, pick[:, None])[:, 0].contiguous()
        envs.advance(actions, reward, done, obs_after, obs_next)
        games.add_(done.sum())

    for _ in range(50):
        advance()
    torch.cuda.synchronize()
    games.zero_()
    began = time.perf_counter()
    for _ in range(args.launches):
        advance()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - began
    print(json.dumps({"form": "one thread per env" if os.environ.get("MZENV_GOMOKU_SERIAL", "0")[:1] not in ("", "0") else "wavefront per env",
                      "envs": E, "launches": args.launches, "host_us_per_launch": 1e6 * seconds / args.launches,
                      "env_moves_per_s": E * args.launches / seconds, "games_finished": int(games.item())}))
    envs.close()


if __name__ == "__main__":
    main()
