#!/bin/bash
# One session on the GPU box: config #5 after mzmcts_downsample_cnn (bench line, kernel stats, root-inference timing) and the CartPole line.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${MZ_OUT_DIR:-$R/measure_out}   # where the measurements go
cd "$R" && mkdir -p "$OUT"
python bench.py --workload atari84 > "$OUT/bench_atari84.json" 2> "$OUT/bench_atari84.err" && cut -c1-200 "$OUT/bench_atari84.json"
python bench.py > "$OUT/bench_cartpole.json" 2> "$OUT/bench_cartpole.err" && cut -c1-200 "$OUT/bench_cartpole.json"
python tools/root_inference_time.py atari84 32768 > "$OUT/root_inference_atari84.json" 2> /dev/null
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/ks_atari84 -o atari84 --output-format csv -- \
    python3 "$R/bench.py" --workload atari84 --steps 4 --warmup 2 --cpu-seconds 0 > "$OUT/ks_atari84.log" 2>&1 \
 && cp "$(find /tmp/ks_atari84 -name '*kernel_stats.csv' | head -1)" "$OUT/atari84_kernel_stats.csv") || exit 1
head -6 "$OUT/atari84_kernel_stats.csv" | cut -c1-160
