#!/bin/bash
cd "$(dirname "$0")/.."; R=$PWD
export OUT=$(realpath -m "${OUT:-bench_logs}")   # where the logs land (any directory; bench_logs/ by default)
mkdir -p $OUT; rm -rf $OUT/prof
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r2 -- python $R/bench.py --steps 1 --warmup 1 --in-flight 1 > $OUT/rocprof_bench.log 2>&1)
echo "rocprof rc=$?"; find $OUT -name "*kernel_trace*" -size +30M -delete 2>/dev/null; ls $OUT/prof; tail -1 $OUT/rocprof_bench.log | cut -c1-200
