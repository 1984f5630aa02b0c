#!/bin/bash
# Re-tune chosen launch shapes of the committed tile caches (after a new tile family became a
# candidate for them) and time the lines with the new choices.  GPU only; outputs under
# $OUT/ (tune_*.json to merge into profiles/, <TAG>_c2 / c4 / c3 bench lines).
# Usage: PATTERN=1/0/5/2/ TAG=r04_s2 bash tools/retune.sh
#   PATTERN: substring of the cache keys to drop (dtype/mode/ksize/stride/...: runtime.prepare)
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
set -e
mkdir -p $OUT
TAG=${TAG:-retune}
PATTERN=${PATTERN:?set PATTERN}
python tools/tune_drop.py profiles/tune_fwd_bf16_b8_256.json $OUT/tin_c2.json $PATTERN
python tools/tune_drop.py profiles/tune_fwd_bf16_b4_1024.json $OUT/tin_c4.json $PATTERN
python tools/tune_drop.py profiles/tune_train_bf16_b16_256.json $OUT/tin_c3.json $PATTERN
timeout -k 10 300 python -u bench.py --full --steps 20 --no-cpu-baseline --tune-cache $OUT/tin_c2.json \
    --save-tune $OUT/tune_fwd_bf16_b8_256.json --layers $OUT/${TAG}_layers_c2.txt \
    > $OUT/${TAG}_c2.json 2> $OUT/${TAG}_c2.err
timeout -k 10 300 python -u bench.py --size 1024 --batch 4 --steps 10 --no-cpu-baseline --no-dp-train \
    --no-parity-mode --tune-cache $OUT/tin_c4.json --save-tune $OUT/tune_fwd_bf16_b4_1024.json \
    > $OUT/${TAG}_c4.json 2> $OUT/${TAG}_c4.err
timeout -k 10 300 python -u bench.py --train --steps 10 --no-cpu-baseline --tune-cache $OUT/tin_c3.json \
    --save-tune $OUT/tune_train_bf16_b16_256.json > $OUT/${TAG}_c3.json 2> $OUT/${TAG}_c3.err
