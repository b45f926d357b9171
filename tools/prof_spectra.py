"""The copy-number spectrum's two sweeps next to their yardsticks, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_spectra.py trace|time       (run on the GPU box; tools/prof_spectra.sh puts `trace` under rocprofv3)

R = the counted read table, A = the assembly counted into a table of its own.
trace: each of these after a warm-up call of the same kind, all in one process so that one kernel trace holds them: histo_kernel over R
       (the streaming yardstick: 16 B per slot), report_scan_kernel over the assembly as ONE sequence (the random-probe yardstick: one
       probe per window), then the spectrum (spectra_reads_kernel over R, spectra_asm_kernel over A)
time:  no profiler: device_seconds of five spectrum calls after a warm-up, their wall time, and the time to count A
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order (the measured call's are the last ones)
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
            if "spectra_" in name or "histo_kernel" in name or "report_scan" in name:
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
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    # two pieces (cut between two reads): a table counted in one piece has its histogram already, and histo_kernel would not run
    cut = (nreads // 2) * (bench.READ_LEN + 1)
    r.count_bases_device(reads.data_ptr(), cut)
    r.count_bases_device(reads.data_ptr() + cut, reads.numel() - cut)
    r.sync()
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    a = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    t0 = time.perf_counter()
    a.count_bases_device(d_asm.data_ptr() if hasattr(d_asm, "data_ptr") else int(d_asm), int(offs[-1]))
    a.sync()
    count_a_wall = time.perf_counter() - t0
    count_a_ms, count_a_launches = a.count_timing()
    ri, ai = r.info(), a.info()
    head = {"mode": mode, "k": bench.K, "bases": asm_len, "thr": thr, "r_slots": ri["slots"], "r_distinct": ri["distinct"], "a_slots": ai["slots"],
            "a_distinct": ai["distinct"], "count_a_wall_s": count_a_wall, "count_a_kernel_ms": count_a_ms, "count_a_launches": count_a_launches}
    if mode == "trace":
        for _ in range(2):
            assert not r.histogram_is_fused()
            r.histogram()
        for _ in range(2):
            rep = r.kmer_report_device(d_asm, [0, offs[-1]], thr)
        for _ in range(2):
            spec = r.spectrum(a)
        head.update({"report_valid_windows": rep.counts[0][1], "report_seconds": rep.seconds, "spectrum_seconds": spec.seconds})
    else:
        secs, wall = [], []
        for _ in range(6):
            t0 = time.perf_counter()
            spec = r.spectrum(a)
            wall.append(time.perf_counter() - t0)
            secs.append(spec.seconds)
        head.update({"spectrum_seconds": secs[1:], "wall_seconds": wall[1:]})
    from jasper_amd import spectra
    solid, found, asm_distinct, asm_only = spectra.derived(spec, thr)
    head.update({"row_sums": [int(x) for x in spec.cells[:, 1:].sum(axis=1)], "asm_only_by_row": [int(x) for x in spec.cells[:, 0]], "solid": solid, "found": found,
                 "completeness": spectra.completeness_pct(found, solid), "asm_distinct": asm_distinct, "asm_only": asm_only})
    print(json.dumps(head))
    a.close()
    r.close()


if __name__ == "__main__":
    main()
