#!/bin/bash
# the whole GPU suite + the NLHE bench lines
OUT=${OUT:?set OUT to the directory for the results}
mkdir -p $OUT
timeout 3000 python -m pytest tests -q -m gpu -x 2>&1 | tail -15 > $OUT/tests.log
cat $OUT/tests.log
for s in external pluribus; do
timeout 900 python bench.py --full --workload nlhe --sampling $s --steps 8 --warmup 4 --cpu-seconds 10 > $OUT/bench_nlhe_$s.json 2> $OUT/bench_nlhe_$s.err
cat $OUT/bench_nlhe_$s.json; tail -2 $OUT/bench_nlhe_$s.err
done
