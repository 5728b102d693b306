#!/bin/bash
# Read bytes and time of the SLICED expand at cfg2 for several builds of the library (tools/build_variant.sh):
#   tools/expand_attribution.sh <tag> <lib.so> [<lib.so> ...]
# Per library: one `rocprofv3 --pmc` run with the three read-request-size counters and nothing else beside them, and one
# separate `rocprofv3 --kernel-trace --stats` run for the kernel times.  Prints one table row per library (read GB of
# pb_expand_kernel from 32 / 64 / 128-byte requests, expand and reduce time); raw output in $ATTR_OUT/attr_<tag>/ (default: build/, which git ignores).
set -u
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ATTR_OUT:-$ROOT/build}/attr_$TAG
mkdir -p $OUT
OUT=$(cd $OUT && pwd)
cd $OUT
BENCH="python3 $ROOT/bench.py --gpus 1 --steps 5 --warmup 2 ${BENCH_ARGS:-}"
for lib in "$@"; do
  name=$(basename $lib .so)
  export SPBLAS_GFX950_LIB=$(cd $ROOT && realpath $lib)
  timeout -k 10 300 rocprofv3 --pmc TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum --output-format csv \
    -d $OUT/pmc_$name -o pmc -- $BENCH > $OUT/pmc_$name.log 2>&1 || { echo "$name: counter run failed ($?)"; exit 1; }
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_$name -o stats -- $BENCH \
    > $OUT/stats_$name.log 2>&1 || { echo "$name: stats run failed ($?)"; exit 1; }
done
cd $ROOT
python3 - "$OUT" "$@" <<'PY'
import csv, glob, os, sys
from collections import defaultdict
out, libs = sys.argv[1], sys.argv[2:]
print("| build | expand read GB | 32 B req | 64 B req | 128 B req | expand us | reduce us |")
print("|---|---|---|---|---|---|---|")
for lib in libs:
    name = os.path.basename(lib)[:-3]
    per = defaultdict(lambda: defaultdict(float))  # dispatch -> counter -> value
    for f in glob.glob(f"{out}/pmc_{name}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "pb_expand_kernel" in r["Kernel_Name"]:
                per[r["Dispatch_Id"]][r["Counter_Name"]] += float(r["Counter_Value"])
    n = max(len(per), 1)
    c = {k: sum(d.get(k, 0.0) for d in per.values()) / n for k in
         ("TCC_EA0_RDREQ_32B_sum", "TCC_EA0_RDREQ_64B_sum", "TCC_EA0_RDREQ_128B_sum")}
    rd = 32 * c["TCC_EA0_RDREQ_32B_sum"] + 64 * c["TCC_EA0_RDREQ_64B_sum"] + 128 * c["TCC_EA0_RDREQ_128B_sum"]
    t = {}
    for f in glob.glob(f"{out}/stats_{name}/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("pb_expand_kernel", "pb_reduce_kernel"):
                if k in r["Name"]:
                    t[k] = float(r["AverageNs"]) / 1e3
    print(f"| {name} | {rd / 1e9:.4f} | {c['TCC_EA0_RDREQ_32B_sum']:.0f} | {c['TCC_EA0_RDREQ_64B_sum']:.0f} | "
          f"{c['TCC_EA0_RDREQ_128B_sum']:.0f} | {t.get('pb_expand_kernel', float('nan')):.1f} | "
          f"{t.get('pb_reduce_kernel', float('nan')):.1f} | (n={len(per)})")
PY
