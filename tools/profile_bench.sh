#!/bin/bash
# The committed evidence of a round (GPU box): bench.py's full JSON line (--full), the rocprofv3 --kernel-trace --stats summary of
# the same command, the CG benchmark and its kernel stats -> OUT_DIR/final_* (copied to profiles/rNN_* by hand).
# Never combines --pmc with tracing; the program itself follows `--`.
# Usage: bash tools/profile_bench.sh OUT_DIR
set -o pipefail
out=$(mkdir -p "${1:?usage: bash tools/profile_bench.sh OUT_DIR}" && cd "$1" && pwd) || exit 1
root=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp && cd "$root"
timeout -k 10 300 python3 bench.py --full > "$out/final_bench.json" 2> "$out/final_bench.err" || echo "bench.py failed"
rm -rf "$out/prof_bench" "$out/prof_cg"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_bench" -- python3 bench.py --full --no-traffic --no-cpu-baseline \
    > "$out/final_bench_under_rocprof.json" 2> "$out/final_bench_under_rocprof.err" || echo "profiled bench failed"
find "$out/prof_bench" -name "*kernel_stats.csv" -exec cp {} "$out/final_bench_kernel_stats.csv" \;
timeout -k 10 300 python3 tools/cg_bench.py --iters 100 2>&1 | grep -v amdgpu.ids > "$out/final_cg.txt" || echo "cg_bench failed"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_cg" -- python3 tools/cg_bench.py --iters 100 \
    > "$out/final_cg_under_rocprof.txt" 2>&1 || echo "profiled cg_bench failed"
find "$out/prof_cg" -name "*kernel_stats.csv" -exec cp {} "$out/final_cg_kernel_stats.csv" \;
rm -rf "$out/prof_bench" "$out/prof_cg"
head -c 600 "$out/final_bench.json"; echo; head -5 "$out/final_bench_kernel_stats.csv"; tail -2 "$out/final_cg.txt"; head -8 "$out/final_cg_kernel_stats.csv"
