#!/bin/bash
# Regenerates the round's judged artifacts under $OUT (default artifacts/; copy to profiles/ afterwards).  GPU box, ~6 min:
#   tools/round_artifacts.sh r02
set -e
tag=$1
cd "$(dirname "$0")/.."
export OUT=${OUT:-artifacts}; mkdir -p $OUT
python3 bench.py --full --dump-launches $OUT/${tag}_bench_launch_shapes.txt 2> $OUT/${tag}_bench.err | tail -1 > $OUT/${tag}_bench_line.json
python3 bench.py --full --precision f32 --no-cpu-baseline 2>> $OUT/${tag}_bench.err | tail -1 > $OUT/${tag}_bench_line_f32.json
python3 bench.py --full --workload config5 --no-cpu-baseline 2>> $OUT/${tag}_bench.err | tail -1 > $OUT/${tag}_bench_line_config5.json
python3 bench.py --full --workload frontend --no-cpu-baseline 2>> $OUT/${tag}_bench.err | tail -1 > $OUT/${tag}_bench_line_frontend.json
echo "bench lines done"
tools/profile_step.sh ${tag}_bf16x6
tools/profile_step.sh ${tag}_f32 --precision f32
echo "kernel traces done"
tools/pmc_passes.sh ${tag}
