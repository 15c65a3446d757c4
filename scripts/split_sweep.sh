#!/bin/bash
# MWB_SPLIT sweep: how many of the cheapest rendered envs a bulk render launch draws as two half-frame workgroups.
# usage: scripts/split_sweep.sh [workload] [split values ...]       (stops at the first run that fails or exceeds its time limit)
set -o pipefail
wl=${1:-maze8192}; [ $# -gt 0 ] && shift
vals=${*:-0 384 768 1152 1536 2048}
for sp in $vals; do
  MWB_SPLIT=$sp timeout -k 10 120 python bench.py --full --no-cpu-baseline --no-vecenv --workload $wl 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$wl split', $sp, round(d['value']/1e6,3), round(d['kernel_ms']['render'],4))" || exit 1
done
