#!/bin/bash
# Diagnostic: the shader clock and socket power the chip holds while bench.py's timed region runs (rocm-smi samples).
#   clock_watch.sh [workload [steps]]     steps: enough for the 12 s of samples (default: six times the workload's own)
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${MZ_OUT_DIR:-$R/measure_out}   # where the measurements go
cd "$R" && mkdir -p "$OUT"
steps=${2:-$(python -c "import bench; print(6 * bench.WORKLOADS['${1:-cartpole}']['steps'])")}
python bench.py --cpu-seconds 0 --steps $steps ${1:+--workload $1} > "$OUT/clock_bench.json" 2> "$OUT/clock_bench.err" &
pid=$!
sleep 2
for i in $(seq 1 30); do
  rocm-smi --showclocks --showpower 2>/dev/null | grep -i -E "sclk|Package Power" | sed -e "s/.*sclk clock level//" -e "s/.*Power (W)//" | tr '\n' ' '; echo
  sleep 0.4
done > "$OUT/clock_samples.txt"
wait $pid
cut -c1-160 "$OUT/clock_bench.json"
cat "$OUT/clock_samples.txt"
