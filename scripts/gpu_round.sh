#!/bin/bash
# One full GPU-box session of a round: the whole GPU suite with its [parity] lines, smoke, the headline bench (+ per-op table),
# the same bench under torchrun with the RCCL path forced on one rank, the small ensembles (per-GPU shards of 2 / 4 / 8 GPUs),
# rocprofv3 kernel stats and - with "pmc" - the two HBM-traffic counter passes.  Everything is bounded by timeouts; logs land in
# $OUT, bench_logs/ by default (copy what is to be judged into profiles/).
export PYTHONUNBUFFERED=1
cd "${GRAFT_REPO_ROOT:-/root/repo}"
R=$PWD
OUT=$(realpath -m "${OUT:-bench_logs}")   # where the logs land (any directory; bench_logs/ by default)
mkdir -p $OUT
: > $OUT/status.log
nproc >> $OUT/status.log; lscpu | grep "Model name" | head -1 >> $OUT/status.log
timeout 1200 python -m pytest tests -m gpu -q -s --timeout=400 --timeout-method=thread > $OUT/t_all.log 2>&1
echo "tests rc=$?" >> $OUT/status.log; tail -1 $OUT/t_all.log >> $OUT/status.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
echo "smoke rc=$?" >> $OUT/status.log
timeout 900 python bench.py --full --steps 12 --warmup 2 --dump-ops $OUT/ops_full.tsv > $OUT/bench_full.json 2> $OUT/bench_full.log
echo "bench rc=$?" >> $OUT/status.log
MARIGOLD_BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 \
  bench.py --full --gpus 1 --steps 10 --warmup 3 --no-cpu-baseline --no-profile > $OUT/bench_nccl_world1.json 2> $OUT/bench_nccl_world1.log
echo "bench nccl rc=$?" >> $OUT/status.log
: > $OUT/small_ensembles.log
for e in 1 2 3 5 8; do
  timeout 300 python bench.py --full --ensemble $e --steps 6 --warmup 2 --no-cpu-baseline --dump-ops $OUT/ops_e$e.tsv 2>/dev/null | python -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        j=json.loads(l); print('E=$e', 'ms_per_map', j['ms_per_step'], 'one_at_a_time', j.get('latency_ms_per_map'), 'stages', {k: round(v['ms'],1) for k,v in j.get('stages',{}).items()}, 'launches', sum(v['launches'] for v in j['kernels'].values()), {k: (round(v['ms'],1), v['launches']) for k,v in j['kernels'].items() if v['ms'] > 1.0})
" >> $OUT/small_ensembles.log
done
echo "small ensembles done" >> $OUT/status.log
# the other configurations of BASELINE.json on one GPU (C2: E = 1 is in the small-ensemble list above)
: > $OUT/configs.log
for cfg in "--scheduler lcm --denoise 4 --ensemble 1" "--kind normals --ensemble 4" "--ensemble 8" "--kind iid --ensemble 1 --denoise 4"; do
  timeout 300 python bench.py --full $cfg --steps 6 --warmup 2 --no-cpu-baseline --no-profile 2>/dev/null | python -c "
import json,sys
for l in sys.stdin:
    if l.startswith('{'):
        j=json.loads(l); print('$cfg |', j['metric'], '|', j['value'], j['unit'], j['ms_per_step'], 'ms', 'one_at_a_time', j.get('latency_ms_per_map'))
" >> $OUT/configs.log
done
echo "configs done" >> $OUT/status.log
rm -rf $OUT/prof
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r6 -- python $R/bench.py --steps 1 --warmup 1 --in-flight 1 > $OUT/rocprof_bench.log 2>&1)
echo "rocprof rc=$?" >> $OUT/status.log
if [ "$1" == "pmc" ]; then
  (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o r6 -- python $R/bench.py --steps 1 --warmup 0 --in-flight 1 > $OUT/pmc_fetch.log 2>&1)
  echo "pmc fetch rc=$?" >> $OUT/status.log
  (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o r6 -- python $R/bench.py --steps 1 --warmup 0 --in-flight 1 > $OUT/pmc_write.log 2>&1)
  echo "pmc write rc=$?" >> $OUT/status.log
fi
find $OUT -name "*kernel_trace*" -size +30M -delete 2>/dev/null
ls -la $OUT/prof/* $OUT/pmc_fetch/* $OUT/pmc_write/* 2>/dev/null | head -20 >> $OUT/status.log
cat $OUT/status.log; cat $OUT/small_ensembles.log; cat $OUT/configs.log
python -c "
import json
for n in ('bench_full','bench_nccl_world1'):
    j=json.loads([l for l in open(f'$OUT/{n}.json') if l.startswith('{')][-1])
    print(n, j['value'], j['ms_per_step'], j.get('roofline'), j.get('collective'), (j.get('calibration') or {}).get('gemm4096_bf16_tflops'))"
