#!/bin/bash
# per-kernel forward times of two library builds on one box (rocprofv3 kernel trace of the
# default bench run): the working tree's library and rgbac/librgbac_hip_prev.so
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
set -e
mkdir -p $OUT
P=$ROOT/deep-learning-based-rgba-image-compression-with-masked-window-based-attention_amd/rgbac/librgbac_hip_prev.so
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof_fwd_new -o fwd -- python3 $ROOT/bench.py --full --steps 20 --no-cpu-baseline --no-dp-train > $OUT/prof_fwd_new.log 2>&1
RGBAC_LIB_PATH=$P timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof_fwd_old -o fwd -- python3 $ROOT/bench.py --full --steps 20 --no-cpu-baseline --no-dp-train > $OUT/prof_fwd_old.log 2>&1
cd $ROOT
for v in new old; do
  python3 tools/prof_db_stats.py $OUT/prof_fwd_$v/fwd_results.db --steps 25 --top 60 --csv $OUT/prof_fwd_$v.csv > $OUT/prof_fwd_$v.txt
  rm -rf $OUT/prof_fwd_$v
done
