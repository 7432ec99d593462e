#!/usr/bin/env python3
"""Kernels and kernel time per training step from two `rocprofv3 --kernel-trace --stats` runs of one way that differ in
their number of steps only (tools/trainer_step_time.py --one-step WAY --steps N): what the longer run has more of, divided
by the difference in steps -- set-up, warm-up and solver searches cancel.  One JSON line.

    kernel_stats_per_step.py LONG.csv SHORT.csv --steps 30 10 --config tictactoe --way "library, eager" [--top 12]
"""
import argparse, csv, json


def read(path):
    with open(path, newline="") as f:
        return {row["Name"]: (int(row["Calls"]), int(row["TotalDurationNs"])) for row in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("long_csv")
    ap.add_argument("short_csv")
    ap.add_argument("--steps", type=int, nargs=2, required=True, metavar=("LONG", "SHORT"))
    ap.add_argument("--config", required=True)
    ap.add_argument("--way", required=True)
    ap.add_argument("--top", type=int, default=12)
    ap.add_argument("--always", default="Conv,conv,Winograd,gemm", help="comma-separated substrings: kernels always listed")
    args = ap.parse_args()
    long_run, short_run = read(args.long_csv), read(args.short_csv)
    steps = args.steps[0] - args.steps[1]
    rows = []
    for name, (calls, ns) in long_run.items():
        calls0, ns0 = short_run.get(name, (0, 0))
        if calls != calls0:
            rows.append({"name": name[:160], "calls_per_step": (calls - calls0) / steps,
                         "us_per_step": round((ns - ns0) / steps / 1e3, 3)})
    rows.sort(key=lambda r: -r["us_per_step"])
    keep = [r for i, r in enumerate(rows) if i < args.top or any(s and s in r["name"] for s in args.always.split(","))]
    print(json.dumps({"source": f"rocprofv3 --kernel-trace --stats of tools/trainer_step_time.py --games {args.config} "
                                f"--one-step WAY, --steps {args.steps[0]} minus --steps {args.steps[1]}, per step",
                      "config": args.config, "way": args.way, "kernels_per_step": sum(r["calls_per_step"] for r in rows),
                      "kernel_us_per_step": round(sum(r["us_per_step"] for r in rows), 2), "kernels": keep}))


if __name__ == "__main__":
    main()
