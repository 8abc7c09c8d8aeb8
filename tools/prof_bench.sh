#!/bin/bash
# rocprofv3 kernel statistics of a bench.py --full run + the line of a second, unprofiled --full run:
#   tools/prof_bench.sh OUTDIR   -> OUTDIR/bench_kernel_stats.csv, OUTDIR/bench.json
OUT=${1:?usage: tools/prof_bench.sh OUTDIR}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -o bench -- python "$R/bench.py" --full > /tmp/bench_prof.log 2>&1
rc=$?
tail -1 /tmp/bench_prof.log | cut -c1-400
[ $rc -eq 0 ] || exit $rc
f=$(find /tmp/prof_bench -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" "$OUT/bench_kernel_stats.csv"
cd "$R" && timeout 600 python bench.py --full 2>/dev/null | tail -1 > "$OUT/bench.json"
cat "$OUT/bench.json"
