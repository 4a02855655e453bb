#!/bin/bash
# The benchmark's full run on a fresh box (python bench.py --full, otherwise the defaults) and its one-line summary;
# usage: bash tools/gpu_bench_default.sh <output dir>; the lines are collected in profiles/r06_bench_default_boxes.jsonl
O=${1:?usage: bash tools/gpu_bench_default.sh <output dir>}
mkdir -p "$O"
t0=$(date +%s)
timeout 900 python bench.py --full > "$O/bench_default_run.json" 2> "$O/bench_default_run.err"
echo "rc=$? wall=$(( $(date +%s) - t0 ))s"
python tools/bench_default_line.py "$O/bench_default_run.json" "$(date -u +%H:%M)" | tee "$O/bench_default_line.json"
