#!/bin/bash
# Kernel stats of porrt_prm_plan_paths: rocprofv3 --kernel-trace --stats of tools/prm_paths_probe.py (one rep per placement, 64 single
# calls) in a run of its own.  Run on the GPU box: bash tools/prm_paths_kstats.sh [outdir]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/out/prm_paths_kstats}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o t -- \
    python3 "$R/tools/prm_paths_probe.py" --reps 1 --singles 64 --out "$OUT/probe_traced.json" > "$OUT/probe_traced.txt" 2> "$OUT/trace.log"
S=$(find "$OUT/trace" -name '*kernel_stats.csv' | head -1)
cp "$S" "$OUT/kernel_stats.csv"
rm -rf "$OUT/trace"
grep -E "k_prm" "$OUT/kernel_stats.csv"
