#!/bin/bash
# run on the GPU box: one kernel trace that holds the read binning kernels and their two yardsticks (hapmer_scan_kernel without a child
# over the same bytes as one contig, and over the same reads as separate sequences), each after a warm-up call; then the calls' own event
# time with the profiler off.  With `e2e` as the second argument: the tool's end-to-end run on all the reads instead; what follows it
# (`--reader device`) is passed on to the tool.  With `gz`: the same workload as one level-6 .fastq.gz through every --gz x --route
# setting of the tool, and the route kernels on one 64 MiB block (`quick` after it: one run of each setting instead of two; `parent=DIR`: a built
# copy of the parent commit's tree, whose tool is run once next to this tree's host / host setting).  Every child of that mode runs under a
# time limit of its own and the first failure ends the run.  With `wgz`: `--write-gz` on that workload (see prof_readbins.py: wgz_e2e).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${1:-prof_readbins_out}      # where the traces and logs go (what is kept of a run is copied to profiles/, see its README)
mkdir -p $OUT
if [ "$2" = "e2e" ]; then
    timeout -k 10 1000 python3 tools/prof_readbins.py e2e "${@:3}" > $OUT/e2e.log 2> $OUT/e2e.err
    rc=$?
    tail -n 5 $OUT/e2e.err; tail -n 2 $OUT/e2e.log
    exit $rc
fi
if [ "$2" = "wgz" ]; then     # --write-gz: the compressor on one 64 MiB block, then the tool with --deflate device, plain + gzip -1, --deflate host
    timeout -k 10 1150 python3 tools/prof_readbins.py wgz > $OUT/wgz.jsonl 2> $OUT/wgz.err
    rc=$?
    tail -n 5 $OUT/wgz.err; cut -c 1-900 $OUT/wgz.jsonl
    exit $rc
fi
if [ "$2" = "gz" ]; then      # the tool on the workload as one .fastq.gz, every --gz x --route setting, and the route kernels on one block
    timeout -k 10 1100 python3 tools/prof_readbins.py gz "${@:3}" > $OUT/gz.jsonl 2> $OUT/gz.err
    rc=$?
    tail -n 5 $OUT/gz.err; cut -c 1-600 $OUT/gz.jsonl
    exit $rc
fi
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 tools/prof_readbins.py trace > $OUT/trace.log 2>&1 &&
timeout -k 10 420 python3 tools/prof_readbins.py time > $OUT/time.log 2>&1
rc=$?
tail -n 3 $OUT/trace.log; tail -n 3 $OUT/time.log
python3 tools/prof_readbins.py summarize $OUT/trace | tee $OUT/summary_trace.json
find $OUT -name '*kernel_stats.csv'
exit $rc
