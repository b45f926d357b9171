#!/bin/bash
# run on the GPU box: kernel traces of one polish call (the yardstick: scan_classify_batch_kernel) and of one dense k-mer report on the
# same text and table, each in a profiling run of its own after a warm-up call; then the report's own event time with the profiler off
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_report_out}      # where the traces and logs go
mkdir -p $OUT
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/polish -- python3 tools/prof_report.py polish > $OUT/polish.log 2>&1 &&
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/report -- python3 tools/prof_report.py report > $OUT/report.log 2>&1 &&
timeout -k 10 200 python3 tools/prof_report.py time > $OUT/time.log 2>&1
rc=$?
tail -3 $OUT/polish.log $OUT/report.log $OUT/time.log
python3 tools/prof_report.py summarize $OUT/polish | tee $OUT/summary_polish.json
python3 tools/prof_report.py summarize $OUT/report | tee $OUT/summary_report.json
find $OUT -name '*kernel_stats.csv'
exit $rc
