#!/bin/bash
# round 6: full -m gpu suite, smoke(), then the default bench line.  Stops at the first failure.
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$ROOT" || exit 1
TAG=${TAG:-a}
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/r06_gputest_$TAG.txt 2>&1 || exit $?
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/r06_smoke_$TAG.txt 2>&1 || exit $?
timeout -k 10 600 python -u bench.py --full > $OUT/r06_line_c2_$TAG.json 2> $OUT/r06_bench_$TAG.err || exit $?
if [ -n "$WITH_TRAIN" ]; then
  timeout -k 10 400 python -u bench.py --full --train > $OUT/r06_line_c3_$TAG.json 2> $OUT/r06_c3_$TAG.err || exit $?
fi
