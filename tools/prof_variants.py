"""The variant scan's kernels next to their yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_variants.py trace|time       (run on the GPU box; tools/prof_variants.sh puts `trace` under rocprofv3)

R = the counted read table, the text = the assembly as ONE sequence, the threshold = the derived one.
trace: each of these after a warm-up call of the same kind, all in one process so that one kernel trace holds them: report_scan_kernel over
       the text (the yardstick: the same tile, ONE random probe per window), then the variant scan (variants_scan_kernel: three probes per
       window; variants_check_kernel: one wave per candidate; variants_compact_kernel)
time:  no profiler: jasper_varscan_seconds of five scans after a warm-up, their wall time, and the report's seconds the same way
       (JASPER_AMD_LIB selects another build of the library: the register variants of DESIGN.md 4.6)
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order (the measured call's are the
       last ones), and the ratio variants_scan_kernel / report_scan_kernel of the last dispatches
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
            if "variants_" in name or "report_" in name or "scan_heads" in name or "scan_stitch" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))
    last = {key: [us[-1] for name, us in out.items() if key in name] for key in ("variants_scan_kernel", "variants_check_kernel", "variants_compact_kernel", "report_scan_kernel")}
    if last["variants_scan_kernel"] and last["report_scan_kernel"]:
        print(json.dumps({key + "_us": round(v[0], 1) for key, v in last.items() if v} |
                         {"ratio": round(last["variants_scan_kernel"][0] / last["report_scan_kernel"][0], 3)}))


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
    import torch
    import bench
    from jasper_amd import KmerTable, polisher
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    ri = r.info()
    text = [0, offs[-1]]
    head = {"mode": mode, "lib": os.environ.get("JASPER_AMD_LIB", ""), "k": bench.K, "bases": asm_len, "thr": thr, "r_slots": ri["slots"], "r_distinct": ri["distinct"]}
    if mode == "trace":
        for _ in range(2):
            rep = r.kmer_report_device(d_asm, text, thr)
        for _ in range(2):
            vs = r.variant_scan_device(d_asm, text, thr)
        head.update({"report_seconds": rep.seconds, "varscan_seconds": vs.seconds})
    else:
        secs, wall, rsecs = [], [], []
        for _ in range(6):
            t0 = time.perf_counter()
            vs = r.variant_scan_device(d_asm, text, thr)
            wall.append(time.perf_counter() - t0)
            secs.append(vs.seconds)
        for _ in range(6):
            rsecs.append(r.kmer_report_device(d_asm, text, thr).seconds)
        head.update({"varscan_seconds": secs[1:], "wall_seconds": wall[1:], "report_seconds": rsecs[1:],
                     "ratio_of_medians": sorted(secs[1:])[2] / sorted(rsecs[1:])[2]})
    head.update({"counts": vs.counts[0], "candidates": vs.candidates, "records": len(vs.records), "retried": vs.retried})
    print(json.dumps(head))
    r.close()


if __name__ == "__main__":
    main()
