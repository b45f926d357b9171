"""The copy-number scan's kernels next to their yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_copies.py trace|time       (run on the GPU box; tools/prof_copies.sh puts `trace` under rocprofv3)

R = the counted read table, A = the assembly counted into a table of its own, the text = the assembly as ONE sequence.
trace: each of these after a warm-up call of the same kind, all in one process so that one kernel trace holds them: report_scan_kernel over
       the text (the yardstick: the same tile, ONE random probe per window), then the copy scan (copies_scan_kernel: two probes per window;
       scan_heads_kernel, scan_stitch_kernel: the dense scans' shared ones)
time:  no profiler: jasper_copyrep_seconds of five scans after a warm-up, and their wall time
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order (the measured call's are the
       last ones), and the ratio copies_scan_kernel / report_scan_kernel of the last dispatches
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
            if "copies_" in name or "report_" in name or "scan_heads" in name or "scan_stitch" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))
    scan = [us for name, us in out.items() if "copies_scan_kernel" in name]
    rep = [us for name, us in out.items() if "report_scan_kernel" in name]
    if scan and rep:
        print(json.dumps({"copies_scan_us": round(scan[0][-1], 1), "report_scan_us": round(rep[0][-1], 1), "ratio": round(scan[0][-1] / rep[0][-1], 3)}))


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
    import torch
    import bench
    from jasper_amd import KmerTable, copies, polisher
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    histo = r.histogram()
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    peak = copies.peak_from_histogram(histo, thr)
    a = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    a.count_bases_device(d_asm.data_ptr() if hasattr(d_asm, "data_ptr") else int(d_asm), int(offs[-1]))
    a.sync()
    ri, ai = r.info(), a.info()
    text = [0, offs[-1]]
    head = {"mode": mode, "lib": os.environ.get("JASPER_AMD_LIB", ""), "k": bench.K, "bases": asm_len, "thr": thr, "peak": peak, "r_slots": ri["slots"],
            "r_distinct": ri["distinct"], "a_slots": ai["slots"], "a_distinct": ai["distinct"]}
    if mode == "trace":
        for _ in range(2):
            rep = r.kmer_report_device(d_asm, text, thr)
        for _ in range(2):
            cr = r.copy_report_device(a, d_asm, text, thr, peak)
        head.update({"report_seconds": rep.seconds, "copyrep_seconds": cr.seconds})
    else:
        secs, wall, rsecs = [], [], []
        for _ in range(6):
            t0 = time.perf_counter()
            cr = r.copy_report_device(a, d_asm, text, thr, peak)
            wall.append(time.perf_counter() - t0)
            secs.append(cr.seconds)
        for _ in range(6):
            rsecs.append(r.kmer_report_device(d_asm, text, thr).seconds)
        head.update({"copyrep_seconds": secs[1:], "wall_seconds": wall[1:], "report_seconds": rsecs[1:],
                     "ratio_of_medians": sorted(secs[1:])[2] / sorted(rsecs[1:])[2]})
    head.update({"counts": cr.counts[0], "runs": len(cr.runs), "excess_runs": int((cr.runs["kind"] == 1).sum()), "retried": cr.retried})
    print(json.dumps(head))
    a.close()
    r.close()


if __name__ == "__main__":
    main()
