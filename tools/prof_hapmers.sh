#!/bin/bash
# run on the GPU box: one kernel trace that holds the hap-mer scan's and census's kernels and their yardsticks (copies_scan_kernel over the
# same text, spectra_reads_kernel over the read table), each after a warm-up call; then the scan's own event time of five calls with the
# profiler off
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_hapmers_out}      # where the traces and logs go (what is kept of a run is copied to profiles/round16/, see its README)
mkdir -p $OUT
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 tools/prof_hapmers.py trace > $OUT/trace.log 2>&1 &&
timeout -k 10 420 python3 tools/prof_hapmers.py time > $OUT/time.log 2>&1
rc=$?
tail -n 3 $OUT/trace.log; tail -n 3 $OUT/time.log
python3 tools/prof_hapmers.py summarize $OUT/trace | tee $OUT/summary_trace.json
find $OUT -name '*kernel_stats.csv'
exit $rc
