#!/bin/bash
# rocprofv3 kernel trace + stats of a few bench steps, reduced to the two summaries that get committed under profiles/:
#   <tag>_kernel_stats.csv (rocprofv3 --stats) and <tag>_timeline.txt (tools/trace_report.py over one step).
# usage (on the GPU box): tools/profile_step.sh <tag> [bench.py arguments...]; results go to $OUT (default artifacts/)
# --full: the per-pattern replays at the end of the run are the steps trace_report.py picks from
set -e
tag=$1; shift
export TMPDIR=/tmp; cd "$(dirname "$0")/.."
dst=${OUT:-artifacts}; mkdir -p $dst
out=$dst/prof_$tag
rm -rf $out
rocprofv3 --kernel-trace --stats --output-format csv -d $out -o run -- python3 bench.py --full --no-cpu-baseline --no-kernel-timing --no-f32-exact --steps 8 --warmup 3 "$@" > $dst/${tag}_bench.log 2>&1
trace=$(find $out -name "*kernel_trace.csv" | head -1)
stats=$(find $out -name "*kernel_stats.csv" | head -1)
python3 tools/trace_report.py "$trace" median 16 > $dst/${tag}_timeline.txt
cp "$stats" $dst/${tag}_kernel_stats.csv
rm -rf $out
tail -1 $dst/${tag}_bench.log | cut -c1-200
