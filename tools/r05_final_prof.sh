#!/bin/bash
# Round-5 closing profile of the default bench command (config 2): rocprofv3 kernel-trace stats
# of that command, the PMC HBM traffic per kernel (separate FETCH_SIZE / WRITE_SIZE passes over
# the forward graph replay), then the bench line reading that traffic summary.  GPU only.
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
set -e
mkdir -p $OUT
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o b -- python bench.py --full --no-cpu-baseline > $OUT/prof_bench.log 2>&1
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o p -- python tools/graph_trace.py --reps 5 > $OUT/pmc_fetch.log 2>&1
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o p -- python tools/graph_trace.py --reps 5 > $OUT/pmc_write.log 2>&1
python tools/pmc_traffic.py $OUT/pmc_fetch/p_counter_collection.csv $OUT/pmc_write/p_counter_collection.csv $OUT/pmc_traffic_fwd.json 8 256
timeout -k 10 400 python bench.py --full --traffic-file $OUT/pmc_traffic_fwd.json > $OUT/bench_final.json 2> $OUT/bench_final.err
