#!/bin/bash
# rocprofv3 kernel-trace + stats of a short bench run; summary copied under gpurun_out/
# usage: bash scripts/prof_stats.sh <tag> [bench args...]
set -e
tag=$1; shift
cd /tmp && export TMPDIR=/tmp
out=$GRAFT_REPO_ROOT/gpurun_out/prof_$tag
rm -rf $out && mkdir -p $out
cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats --output-format csv -d $out -- python3 bench.py --full --no-cpu-baseline "$@" > $out/bench.log 2>&1
find $out -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $out/kernel_stats.csv
python3 - $out/kernel_stats.csv <<PY
import csv, sys
for r in list(csv.DictReader(open(sys.argv[1])))[:24]:
    print("%-66s calls %5s avg %9.1f us total %8.2f ms %6s%%" % (r["Name"][:66], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6, r["Percentage"]))
PY
tail -1 $out/bench.log | cut -c1-400
