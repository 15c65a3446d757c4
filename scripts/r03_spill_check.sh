#!/bin/bash
# round 3, after the spill removal: GPU tests, bench lines of the workloads whose kernels changed, PMC traffic of YMaze / PutNext
set -o pipefail
out=${1:?usage: scripts/r03_spill_check.sh <output dir>}; mkdir -p $out
python -m pytest tests -m gpu -x -q > $out/gputests.log 2>&1; echo "gpu tests rc=$?"; tail -3 $out/gputests.log
for wl in ymaze8192 putnext8192 tmaze_features8192 maze8192; do
  python bench.py --full --workload $wl --no-cpu-baseline > $out/bench_$wl.json 2> $out/bench_$wl.err || echo "bench $wl failed"
  python -c "import json;d=json.load(open('$out/bench_$wl.json'));print('$wl',round(d['value']/1e6,3),d['kernel_ms'])"
done
for wl in ymaze8192 putnext8192; do
  bash scripts/profile_workload.sh r03 $wl > $out/prof_$wl.log 2>&1 || echo "profile $wl failed"
  tail -1 $out/prof_$wl.log | cut -c1-300
done
