#!/bin/bash
# Same-box A/B of two builds of the library through the bench's per-layer detail (base, new, base, new, ...):
#   [REPS=3] tools/ab_libs.sh tag [layer-name-regex]
# Every bench run has its own time limit, and the first one that fails ends the script.
set -o pipefail
tag=${1:-ab}; pat=${2:-.}
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}      # results folder, relative to the repository root
mkdir -p "$OUT"
for rep in $(seq 1 ${REPS:-2}); do
  for which in base new; do
    lib=values_amd/libvalues_amd.so; [ $which = base ] && lib=values_amd/libvalues_amd_base.so
    VX_LIB_PATH=$lib timeout -k 10 240 python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-latency --no-storage16 --detail $OUT/${tag}_${which}_layers.json 2>/dev/null | python3 -c "
import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$which', d['value'], d['ms_per_step'])" || exit 1
  done
done
for which in base new; do echo "== $which"; python3 tools/show_layers.py $OUT/${tag}_${which}_layers.json | grep -E "$pat"; done
