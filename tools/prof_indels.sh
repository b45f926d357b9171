#!/bin/bash
# run on the GPU box: one kernel trace that holds the variant scan's kernels (the yardstick: variants_check_kernel, 2k lookups per
# candidate) and indels_check_kernel at max_len 4 and 16, each after a warm-up call; then the indel scan's own event time of five calls
# with the profiler off
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_indels_out}      # where the traces and logs go
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 tools/prof_indels.py trace > $OUT/trace.log 2>&1 &&
timeout -k 10 300 python3 tools/prof_indels.py time > $OUT/time.log 2>&1
rc=$?
tail -n 3 $OUT/trace.log $OUT/time.log
python3 tools/prof_indels.py summarize $OUT/trace $OUT/trace.log | tee $OUT/summary_trace.json
# the mixed half: a trace of its own (indels_mixed_kernel next to indels_check_kernel on the same candidates), then its event time
if [ $rc -eq 0 ]; then
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_mixed -- python3 tools/prof_indels.py trace_mixed > $OUT/trace_mixed.log 2>&1 &&
    timeout -k 10 300 python3 tools/prof_indels.py time_mixed > $OUT/time_mixed.log 2>&1
    rc=$?
    tail -n 3 $OUT/trace_mixed.log $OUT/time_mixed.log
    python3 tools/prof_indels.py summarize_mixed $OUT/trace_mixed $OUT/trace_mixed.log | tee $OUT/summary_trace_mixed.json
fi
# the het-cluster half: a trace of its own (het_cluster_kernel next to indels_mixed_kernel at max_len 16 on the same candidates), its event
# time, and the diploid leg
if [ $rc -eq 0 ]; then
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_clusters -- python3 tools/prof_indels.py trace_clusters > $OUT/trace_clusters.log 2>&1 &&
    timeout -k 10 300 python3 tools/prof_indels.py time_clusters > $OUT/time_clusters.log 2>&1 &&
    timeout -k 10 300 python3 tools/prof_indels.py diploid_clusters > $OUT/diploid_clusters.log 2>&1
    rc=$?
    tail -n 3 $OUT/trace_clusters.log $OUT/time_clusters.log $OUT/diploid_clusters.log
    python3 tools/prof_indels.py summarize_clusters $OUT/trace_clusters $OUT/trace_clusters.log | tee $OUT/summary_trace_clusters.json
fi
find $OUT -name '*kernel_stats.csv'
exit $rc
