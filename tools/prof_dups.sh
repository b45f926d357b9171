#!/bin/bash
# run on the GPU box: the duplication map's two kernels and their yardstick (copies_scan_kernel over the same text and tables) in one
# process with the profiler off: HIP-event medians of five calls after a warm-up (tools/prof_dups.py)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_dups_out}      # where the log goes
mkdir -p $OUT
timeout -k 10 420 python3 tools/prof_dups.py time > $OUT/time.log 2>&1
rc=$?
tail -3 $OUT/time.log
exit $rc
