#!/bin/bash
# the two PMC passes of scripts/gpu_round.sh (HBM traffic per kernel), alone
cd "$(dirname "$0")/.."; R=$PWD
export OUT=$(realpath -m "${OUT:-bench_logs}")   # where the logs land (any directory; bench_logs/ by default)
mkdir -p $OUT; rm -rf $OUT/pmc_fetch $OUT/pmc_write
(cd /tmp && export TMPDIR=/tmp && timeout 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o r2 -- python $R/bench.py --steps 1 --warmup 0 --in-flight 1 > $OUT/pmc_fetch.log 2>&1); echo "pmc fetch rc=$?"
(cd /tmp && export TMPDIR=/tmp && timeout 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o r2 -- python $R/bench.py --steps 1 --warmup 0 --in-flight 1 > $OUT/pmc_write.log 2>&1); echo "pmc write rc=$?"
