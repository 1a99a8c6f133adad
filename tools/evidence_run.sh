#!/bin/bash
# Evidence run on the GPU box (one script for every round; the per-round one-off scripts of r3 are gone):
#   tools/evidence_run.sh <tag> [quick]
# suite, the --full bench line (+ live traffic and MFMA-busy PMC passes), rocprofv3 --kernel-trace --stats summaries of the
# default command with the GEMM table and of the step loop alone; without `quick` also the HBM-bound kernels and decode tables.
# Everything lands in $OUT/<tag>_* (OUT: a folder under the repo root, default evidence_out/); copy what is to be judged into profiles/.
TAG=${1:-r04_a}; MODE=${2:-full}
cd "$(dirname "$0")/.."
OUT=${OUT:-evidence_out}
mkdir -p $OUT
( CS_PARITY_LOG=$PWD/$OUT/${TAG}_parity_log.txt timeout 1500 python -m pytest tests -m gpu -q -x --durations=8 > $OUT/${TAG}_tests.log 2>&1; echo "pytest rc=$?" >> $OUT/${TAG}_tests.log )
tail -14 $OUT/${TAG}_tests.log
timeout 1200 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"
tail -3 $OUT/${TAG}_bench.err
python - <<PY
import json
try:
    d = json.load(open('$OUT/${TAG}_bench.json')); r = d['roofline']
    print('steps/s', d['value'], 'ms', d['ms_per_step'], 'frac', r['frac'], 'avg_ms', r['avg_launch_ms'], 'traffic', r['traffic'],
          'busy', r.get('mfma_busy_frac'), 'clk', r.get('effective_clock_ghz'))
    print('c2', d['c2']['ms_per_step'], 'c7', d['c7']['ms_per_step'], d['c7']['ms_per_object_step'], 'decode/obj', d['decode']['ms_per_object'])
    print('c7x5', json.dumps(d.get('c7x5')))
    print('cpu', d['cpu_baseline']['value'], 'fp32', d['fp32_mfma']['value'])
    print('busy detail', json.dumps(r.get('mfma_busy_detail')))
except Exception as e:
    print('no bench line', e)
PY
REPO=$(pwd)
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $REPO/$OUT/prof_${TAG} -o bench -- python $REPO/bench.py --full --no-cpu-baseline --no-traffic --gemm-table > $REPO/$OUT/${TAG}_bench_under_rocprof.json 2> $REPO/$OUT/${TAG}_gemm_table.txt
timeout 600 rocprofv3 --kernel-trace --stats -d $REPO/$OUT/prof_${TAG}2 -o bench -- python $REPO/bench.py --full --no-cpu-baseline --no-extras > $REPO/$OUT/${TAG}_bench_steploop_under_rocprof.json 2> /dev/null
timeout 600 rocprofv3 --kernel-trace --stats -d $REPO/$OUT/prof_${TAG}3 -o bench -- python $REPO/bench.py --full --no-cpu-baseline --no-extras --objects 1 --steps 20 --warmup 3 > $REPO/$OUT/${TAG}_bench_c2_under_rocprof.json 2> /dev/null
timeout 600 rocprofv3 --kernel-trace --stats -d $REPO/$OUT/prof_${TAG}4 -o bench -- python $REPO/bench.py --full --no-cpu-baseline --no-traffic --no-extras --objects 7 --steps 10 --warmup 3 --gemm-table > $REPO/$OUT/${TAG}_bench_c7_under_rocprof.json 2> $REPO/$OUT/${TAG}_gemm_table_c7.txt
cd $REPO
DB=$(find $OUT/prof_${TAG}4 -name "*.db" | head -1)
[ -n "$DB" ] && python tools/rocpd_summary.py $DB > $OUT/${TAG}_c7_kernel_stats.txt
grep -v "^[WEI]2026" $OUT/${TAG}_gemm_table_c7.txt | head -45 > $OUT/${TAG}_gemm_table_c7_clean.txt
DB=$(find $OUT/prof_${TAG} -name "*.db" | head -1)
[ -n "$DB" ] && python tools/rocpd_summary.py $DB > $OUT/${TAG}_kernel_stats.txt
DB=$(find $OUT/prof_${TAG}2 -name "*.db" | head -1)
[ -n "$DB" ] && python tools/rocpd_summary.py $DB > $OUT/${TAG}_kernel_stats_steploop.txt && python tools/rocpd_by_grid.py $DB "conv_gemm_f16x3_kernel<1, 7, 8, 1, true, 32," > $OUT/${TAG}_dominant_kernel_by_grid.txt && head -8 $OUT/${TAG}_kernel_stats_steploop.txt | cut -c1-170
DB=$(find $OUT/prof_${TAG}3 -name "*.db" | head -1)
[ -n "$DB" ] && python tools/rocpd_summary.py $DB > $OUT/${TAG}_c2_kernel_stats.txt
rm -rf $OUT/prof_${TAG} $OUT/prof_${TAG}2 $OUT/prof_${TAG}3 $OUT/prof_${TAG}4
grep -v "^[WEI]2026" $OUT/${TAG}_gemm_table.txt | head -45 > $OUT/${TAG}_gemm_table_clean.txt
if [ "$MODE" != "quick" ]; then
  python tools/hbm_bench.py > $OUT/${TAG}_hbm_bound_kernels.txt 2>&1
  python tools/decode_bench.py > $OUT/${TAG}_decode_table.txt 2>&1
  for nb in 2 14 64; do SM_BATCH=$nb timeout 600 python tools/gemm_tok_smallm.py > $OUT/${TAG}_tok_smallm_b$nb.txt 2>&1; done
  SM_BATCH=2 timeout 600 python tools/gemm_smallm_tiles.py > $OUT/${TAG}_smallm_tiles_b2.txt 2>&1
  head -3 $OUT/${TAG}_decode_table.txt
fi
