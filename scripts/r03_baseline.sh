#!/bin/bash
# round-3 baseline: headline line, isolated stage times, the lane kernel's own cycle split
# usage: bash scripts/r03_baseline.sh [OUTDIR]
set -e
OUT=${1:-r03_baseline}
mkdir -p $OUT
python bench.py --steps 5 --warmup 2 --full --e2e-frames 0 --no-cpu-baseline > $OUT/base_bench.json 2> $OUT/base_bench.err
cat $OUT/base_bench.json
JXLHIP_LANES_PROF=1 python bench.py --no-pipeline --steps 2 --warmup 1 --full --e2e-frames 0 --no-cpu-baseline > $OUT/base_prof.json 2> $OUT/base_prof.err
grep "lanes prof" $OUT/base_prof.err | tail -3
cat $OUT/base_prof.json
