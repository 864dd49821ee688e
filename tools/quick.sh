#!/bin/bash
# one gpurun call: a test subset + the default step with its per-shape table.  QUICK_TESTS="tests/x.py -k expr" tools/quick.sh
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-run_out}      # where the results go (relative to the repository root)
mkdir -p $OUT
if [ -n "$QUICK_TESTS" ]; then timeout 900 python -m pytest $QUICK_TESTS -m gpu -x -q --tb=short 2>&1 | tail -8; fi
if [ -z "$NO_BENCH" ]; then
BENCH_SHAPE_TABLE=$OUT/quick_shape_table.txt timeout 600 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-traffic --no-extras 2>/dev/null | tail -1 | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print('ms_per_step', d['ms_per_step'], 'roofline', d['roofline']['achieved'])"
head -32 $OUT/quick_shape_table.txt
fi
