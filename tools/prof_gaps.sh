#!/bin/bash
# run on the GPU box: the gap scan on the 47 Mb measurement workload with about 1 000 planted gaps, at --gap-max-len 1000 and 4096, next
# to the compound search on the same text -- the library's own event times, no profiler (tools/prof_gaps.py)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_gaps_out}      # where the log goes
mkdir -p $OUT
timeout -k 10 600 python3 tools/prof_gaps.py > $OUT/time.log 2>&1
rc=$?
tail -n 3 $OUT/time.log
exit $rc
