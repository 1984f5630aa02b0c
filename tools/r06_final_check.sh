#!/bin/bash
# Final check of the in-tree library at HEAD: the -m gpu suite, smoke(), the default bench line.
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$ROOT" || exit 1
set -e
mkdir -p $OUT
T=${T:-r06l}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/${T}_gputest.txt 2>&1
tail -n 1 $OUT/${T}_gputest.txt
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.txt 2>&1
tail -n 2 $OUT/${T}_smoke.txt
timeout -k 10 400 python -u bench.py --full > $OUT/${T}_c2.json 2> $OUT/${T}_c2.err
echo "c2: $(cut -c 90-190 $OUT/${T}_c2.json)"
