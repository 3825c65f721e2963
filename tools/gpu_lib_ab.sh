#!/bin/bash
# A/B of two builds of the engine on the per-GPU tiles (tools/torus_bench.py) and on the bench grid:
#   new = climate-sim-mpi-cpp_amd/lib/libcsim.so, old = $OLD_LIB (another build of the engine)
# interleaved twice so that box drift shows.  Output: gpurun_out/lib_ab.jsonl
# ROUNDS, SHAPES, STEPS, RUNS and MODES change that.  Defaults: two rounds, 1200 steps on the 8-GPU tiles with and without the self-linked exchange, 20-step calls and one
# long run.  ORDER="old new" runs the other build first in every pair (default: new old).  A kernel-only comparison: ROUNDS=5 SHAPES="16384x16384 4096x8192" STEPS=420 RUNS=0 MODES=single
set -o pipefail
R=${GRAFT_REPO_ROOT:-$PWD}
OLD=${OLD_LIB:?set OLD_LIB to the other build of libcsim.so (e.g. make OUT=../lib_old/libcsim.so OBJDIR=../build_old in a checkout of the other revision)}
ROUNDS=${ROUNDS:-2}
SHAPES=${SHAPES:-4096x8192 8192x8192}
STEPS=${STEPS:-1200}
RUNS=${RUNS:-20 0}
MODES=${MODES:-single torus-auto}
ORDER=${ORDER:-new old}
out=$R/gpurun_out/lib_ab.jsonl
mkdir -p $(dirname $out)
: > $out
for rnd in $(seq 1 $ROUNDS); do
  for v in $ORDER; do
    if [ $v = old ]; then export CSIM_LIB=$OLD; else unset CSIM_LIB; fi
    for run in $RUNS; do
      timeout -k 10 300 python3 $R/tools/torus_bench.py --shape $SHAPES --steps $STEPS --run $run --modes $MODES 2>/dev/null \
        | sed "s/^{/{\"lib\": \"$v\", \"round\": $rnd, /" >> $out || exit 1
    done
    timeout -k 10 300 python3 $R/bench.py --gpus 1 --no-cpu-baseline --steps 20 --warmup 5 2>/dev/null | python3 -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
print(json.dumps({'lib': '$v', 'round': $rnd, 'bench': '16384x16384 --steps 20', 'mcells': d['value'], 'repeats_ms_per_step': d['config'].get('repeats_ms_per_step'),
                  'kernel_avg_ms': (d.get('roofline') or {}).get('kernel_avg_ms'),
                  'rows_per_chunk_last_launch': d['config'].get('rows_per_chunk_last_launch'), 'preflight_ok': (d['config'].get('parity_preflight') or {}).get('ok')}))" >> $out || exit 1
  done
done
cat $out
