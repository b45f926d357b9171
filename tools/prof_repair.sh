#!/bin/bash
# run on the GPU box: the repair stage's event times with the profiler off (the apply kernel next to a device-to-device copy of the same
# text, the stage next to the scans it calls), then one kernel trace (no counters) of two repair calls
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_repair_out}      # where the traces and logs go
mkdir -p $OUT
timeout -k 10 400 python3 tools/prof_repair.py time > $OUT/time.log 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 tools/prof_repair.py trace > $OUT/trace.log 2>&1 &&
timeout -k 10 60 python3 tools/prof_repair.py summarize $OUT/trace > $OUT/summary_trace.json
rc=$?
tail -n 3 $OUT/time.log $OUT/trace.log $OUT/summary_trace.json
find $OUT -name '*kernel_stats.csv'
exit $rc
