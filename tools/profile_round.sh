#!/bin/bash
# One profiling session on the GPU box for profiles/<round>/: kernel trace + stats of a plain bench run
# (no property / assembly / config / PCIe legs, so the per-kernel rows describe only the config-5 decode
# launch), launch spans, FETCH_SIZE and WRITE_SIZE in separate --pmc passes (-> profiles/pmc_traffic.json,
# which the bench line's roofline.traffic reads), then the full bench line (bench.py --full).
# Every GPU step has its own time limit; the chain stops at the first failure.
# usage: tools/profile_round.sh [ROUND]   output under $COVT_PROFILE_OUT (default profile_out/)
set -euo pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
R=${1:-r03}
OUT=${COVT_PROFILE_OUT:-profile_out}
mkdir -p "$OUT/$R"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- \
    python bench.py --steps 20 --warmup 3 > "$OUT/$R/prof_bench.json" 2> "$OUT/$R/prof_bench.err"
python tools/launch_span.py "$OUT/prof/run_kernel_trace.csv" > "$OUT/$R/rocprof_launch_spans.txt"
cp "$OUT/prof/run_kernel_stats.csv" "$OUT/$R/rocprof_kernel_stats.csv"
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE -d "$OUT/pmc_fetch" -o run --output-format csv -- \
    python bench.py --steps 3 --warmup 1 > /dev/null 2> "$OUT/$R/pmc_fetch.err"
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE -d "$OUT/pmc_write" -o run --output-format csv -- \
    python bench.py --steps 3 --warmup 1 > /dev/null 2> "$OUT/$R/pmc_write.err"
python tools/pmc_traffic.py "$OUT" > "$OUT/$R/pmc_traffic.txt"
cp profiles/pmc_traffic.json "$OUT/$R/pmc_traffic.json"
timeout -k 10 600 python bench.py --full > "$OUT/$R/bench.json" 2> "$OUT/$R/bench.err"
timeout -k 10 300 python tools/config_timeline.py > "$OUT/$R/config_timeline.txt" 2>&1
timeout -k 10 300 python tools/op_breakdown.py > "$OUT/$R/op_breakdown.txt" 2>&1
OPB_PROPS=1 timeout -k 10 300 python tools/op_breakdown.py > "$OUT/$R/op_breakdown_props.txt" 2>&1
echo "profile session done"
