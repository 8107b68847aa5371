#!/bin/bash
# usage (GPU box, repo root): tools/r6_final.sh <tag>  -- the round's closing run: the driver's bench command on the fresh box, C4 both workloads, then the
# GPU test suite (a bench that FOLLOWS the suite on one box runs its end-to-end leg at half the rate: page cache full of the tests' files)
TAG=$1
OUT=${OUT:-out}  # logs and bench lines go here
mkdir -p $OUT
timeout 1500 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench_driver.json 2> $OUT/${TAG}_bench_driver.err; echo "bench rc=$?"
python3 tools/bench_line.py c2 < $OUT/${TAG}_bench_driver.json | cut -c1-600; tail -2 $OUT/${TAG}_bench_driver.err
timeout 1500 python3 bench.py --full --config c4 --steps 8 --warmup 2 --no-end-to-end > $OUT/${TAG}_bench_c4.json 2> $OUT/${TAG}_bench_c4.err; echo "bench c4 rc=$?"
python3 tools/bench_line.py c4 < $OUT/${TAG}_bench_c4.json | cut -c1-600
timeout 2400 python3 -m pytest tests -m gpu -x -q > $OUT/${TAG}_pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $OUT/${TAG}_pytest_gpu.log
tail -6 $OUT/${TAG}_pytest_gpu.log
