#!/bin/bash
# kernel trace of the config-3 training bench; one graph-replayed step's kernels summarised on
# the box (the step = the dispatches between the last two mse_bwd_kernel launches)
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
set -e
mkdir -p $OUT
R=$ROOT
T=${1:-train}
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof_$T -o t -- python3 $R/bench.py --full --train --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_$T.log 2>&1
cd $R
python3 tools/prof_db_stats.py $OUT/prof_$T/t_results.db --step-marker mse_bwd_kernel --top 70 --csv $OUT/prof_$T.csv > $OUT/prof_$T.txt
rm -rf $OUT/prof_$T
