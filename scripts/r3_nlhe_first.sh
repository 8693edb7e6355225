#!/bin/bash
# round 3, first GPU contact of the level-synchronous NLHE traversal: parity tests, then the bench at three batch sizes
OUT=${OUT:?set OUT to the directory for the results}
mkdir -p $OUT
timeout 1500 python -m pytest tests/test_gpu_nlmc.py tests/test_gpu_nlhe.py "tests/test_golden.py::test_device_reproduces_nlmc_golden" -x -q -m gpu 2>&1 | tail -25 > $OUT/tests.log
cat $OUT/tests.log
for b in 128 16384 262144; do
  timeout 600 python bench.py --full --workload nlhe --nlhe-batch $b --steps 6 --warmup 2 --cpu-seconds 0 > $OUT/bench_$b.json 2> $OUT/bench_$b.err
  tail -c 1500 $OUT/bench_$b.json; tail -3 $OUT/bench_$b.err
done
