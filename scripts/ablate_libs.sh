#!/bin/bash
# Timing ablations: the bench (no CPU baseline, no rollout unless $ROLL) with each diagnostic library in $LIBS;
# logs go to the folder $OUT_DIR names.
set -euo pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:?folder for the logs}
mkdir -p "$O"
for L in ${LIBS}; do
  HK_LIB=hockey-env_amd/hockey_amd/_lib/$L timeout -k 10 120 python bench.py --full --no-cpu-baseline --rollout ${ROLL:-0} --steps 300 --warmup 200 > "$O/abl_$L.log" 2>&1
  echo "$L $(grep -o '"kernel_avg_ms": [0-9.e+]*' "$O/abl_$L.log") $(grep -o '"rollout": {[^}]*}' "$O/abl_$L.log" | grep -o '"ms_per_step": [0-9.]*')"
done
