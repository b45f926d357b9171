#!/bin/bash
# run on the GPU box: one kernel trace (no counters) that holds compound_search_kernel at max_len 64 and its yardstick, indels_mixed_kernel
# at max_len 16, each after a warm-up call; then the search's own event time of five calls with the profiler off
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_compound_out}      # where the traces and logs go
mkdir -p $OUT
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 tools/prof_compound.py trace > $OUT/trace.log 2>&1 &&
timeout -k 10 400 python3 tools/prof_compound.py time > $OUT/time.log 2>&1 &&
timeout -k 10 60 python3 tools/prof_compound.py summarize $OUT/trace $OUT/trace.log > $OUT/summary_trace.json
rc=$?
tail -n 3 $OUT/trace.log $OUT/time.log $OUT/summary_trace.json
find $OUT -name '*kernel_stats.csv'
exit $rc
