#!/bin/bash
# One session on the GPU box: the whole GPU suite, then the four bench lines (profiles/r03_bench_*.json).
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${MZ_OUT_DIR:-$R/measure_out}   # where the measurements go
cd "$R" && mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -q -m gpu -x > "$OUT/gpu_suite.log" 2>&1; rc=$?; echo "pytest rc=$rc" >> "$OUT/gpu_suite.log"
tail -3 "$OUT/gpu_suite.log"
[ $rc -eq 0 ] || exit $rc
for w in cartpole tictactoe atari84 connect4; do
  python bench.py --workload $w > "$OUT/bench_$w.json" 2> "$OUT/bench_$w.err" && echo "$w: $(cut -c1-150 "$OUT/bench_$w.json")"
done
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1; tail -1 "$OUT/smoke.log"
