#!/bin/bash
# Instruction mix and memory traffic of the bulk render kernel: two --pmc passes (SQ instruction counts + FETCH_SIZE, then WRITE_SIZE; the
# two TCC counters do not fit one pass), nothing else traced.  MWB_LIB selects the library, so a parent build can be counted beside the tree's.
# usage: scripts/fetch_counters.sh <out.json> [workload]
set -eo pipefail
OUTJ=${1:?out.json}; WL=${2:-maze8192}
cd "$(dirname "$(readlink -f "$0")")/.."
P=$(mktemp -d "${TMPDIR:-/tmp}/fetch_counters.XXXXXX")
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES FETCH_SIZE --output-format csv -d $P/a -- python3 bench.py --workload $WL --steps 20 --warmup 5 > $P.a.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $P/b -- python3 bench.py --workload $WL --steps 20 --warmup 5 > $P.b.log 2>&1
python3 - "$P" "$OUTJ" "$WL" <<'PY'
import csv, glob, collections, json, sys
agg = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/*/*/*_counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        if "render_kernel<256, 2" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
out = {"workload": sys.argv[3], "kernel": "render_kernel<256, 2, ...> (bulk launch), mean per launch", "launches": len(next(iter(agg.values()))) if agg else 0,
       "counters": {k: round(sum(v) / len(v), 1) for k, v in sorted(agg.items())}}
json.dump(out, open(sys.argv[2], "w"), indent=1, sort_keys=True)
print(json.dumps(out))
PY
rm -rf $P $P.a.log $P.b.log
