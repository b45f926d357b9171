"""The dense k-mer report next to its yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_report.py polish|report|time       (run on the GPU box; tools/prof_report.sh puts the first two under rocprofv3)

polish: a warm-up polish call, then one more -- the yardstick is scan_classify_batch_kernel (pass 0's dense scan: one lookup per
        window of the same text) in the kernel trace of that last call
report: a warm-up report, then one more over the same text as ONE sequence, same table and threshold
time:   no profiler: jasper_report_seconds of five reports after a warm-up, and the wall time of the calls
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order (the last call's are the last ones)
"""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(d):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            if "report_" in name or "scan_heads" in name or "scan_stitch" in name or "scan_classify" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
    import torch
    import bench
    from jasper_amd import KmerTable, polisher
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    t = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    t.count_bases_device(reads.data_ptr(), reads.numel())
    t.sync()
    thr = int(polisher.threshold_from_histo_rows(t.histo_rows())[0])
    whole = [0, offs[-1]]
    if mode == "polish":
        for _ in range(2):
            res = t.polish_batch_device(d_asm, offs, thr, 2, fix=True)
        print(json.dumps({"mode": mode, "bases": asm_len, "thr": thr, "polish_dev_s": res.seconds}))
    else:
        n = 2 if mode == "report" else 6
        secs, wall = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            rep = t.kmer_report_device(d_asm, whole, thr)
            wall.append(time.perf_counter() - t0)
            secs.append(rep.seconds)
        tot = rep.counts[0]
        print(json.dumps({"mode": mode, "lib": os.environ.get("JASPER_AMD_LIB", ""), "bases": asm_len, "thr": thr, "counts": tot, "runs": len(rep.runs), "retried": rep.retried,
                          "report_seconds": secs[1:], "wall_seconds": wall[1:], "gbp_per_s": [asm_len / s / 1e9 for s in secs[1:]]}))
    t.close()


if __name__ == "__main__":
    main()
