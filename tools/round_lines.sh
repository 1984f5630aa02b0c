# Round bench lines (GPU only; outputs under $OUT/<TAG>_*): smoke, config 2 (default: CPU
# baseline, fp32 parity line with symbol accounting, dp_train sub-record), config 1 (--alpha),
# config 3 (--train), config 4 (--size 1024 --batch 4), the RGBA pipeline (--rgba).
ROOT=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-$ROOT/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
set -e
mkdir -p $OUT
TAG=${TAG:-r03}
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_c2.json 2> $OUT/${TAG}_c2.err
timeout -k 10 300 python bench.py --full --alpha > $OUT/${TAG}_c1.json 2> $OUT/${TAG}_c1.err
timeout -k 10 400 python bench.py --full --train > $OUT/${TAG}_c3.json 2> $OUT/${TAG}_c3.err
timeout -k 10 500 python bench.py --full --size 1024 --batch 4 --no-dp-train > $OUT/${TAG}_c4.json 2> $OUT/${TAG}_c4.err
timeout -k 10 300 python bench.py --full --rgba --no-cpu-baseline > $OUT/${TAG}_rgba.json 2> $OUT/${TAG}_rgba.err
