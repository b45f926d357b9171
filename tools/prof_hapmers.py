"""The hap-mer scan's and census's kernels next to their yardsticks, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37).

    python tools/prof_hapmers.py trace|time       (run on the GPU box; tools/prof_hapmers.sh puts `trace` under rocprofv3)

R = the counted read table (the child), A = the assembly counted into a table of its own, the text = the assembly as ONE sequence.  The two
"parents" are two copies of the assembly with independent substitutions at 0.1 %; M and P = each copy's reads at 30x, counted.
trace: each of these after a warm-up call of the same kind, all in one process so that one kernel trace holds them: the copy scan over the
       text (copies_scan_kernel, the scan's yardstick: the same tile, two unconditional probes per window), the spectrum (spectra_reads_kernel,
       the census's yardstick: one sweep over a read table's slots with one probe per key), then the hap-mer scan (hapmer_scan_kernel;
       scan_heads_kernel, scan_stitch_kernel: the dense scans' shared ones) and the census (hapmer_census_kernel, twice)
time:  no profiler: jasper_hapscan_seconds of five scans after a warm-up, the same of the copy scan, and the census's and the spectrum's seconds
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR, the durations of its dispatches in order (the measured call's are the
       last ones), and the ratios hapmer_scan_kernel / copies_scan_kernel and hapmer_census_kernel / spectra_reads_kernel of the last dispatches
"""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SNP = 0.001


def summarize(d):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            name = r["Kernel_Name"].split("(")[0]
            if "copies_" in name or "hapmer_" in name or "spectra_" in name or "scan_heads" in name or "scan_stitch" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))

    def last(what, n=1):
        us = [v for name, v in out.items() if what in name]
        return us[0][-n:] if us else None
    scan, cop, cen, spec = last("hapmer_scan_kernel"), last("copies_scan_kernel"), last("hapmer_census_kernel", 2), last("spectra_reads_kernel")
    if scan and cop:
        print(json.dumps({"hapmer_scan_us": round(scan[0], 1), "copies_scan_us": round(cop[0], 1), "ratio": round(scan[0] / cop[0], 3)}))
    if cen and spec:
        print(json.dumps({"hapmer_census_us": [round(x, 1) for x in cen], "spectra_reads_us": round(spec[0], 1), "ratio_per_parent": [round(x / spec[0], 3) for x in cen]}))


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
    import torch
    import bench
    from jasper_amd import KmerTable, copies, polisher, synth
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    slots = max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10))      # (sized as bench.py sizes it)
    r = KmerTable(bench.K, min_slots=slots)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    del reads
    thr = int(polisher.threshold_from_histo_rows(r.histo_rows())[0])
    peak = copies.peak_from_histogram(r.histogram(), thr)
    a = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    a.count_bases_device(d_asm.data_ptr(), int(offs[-1]))
    a.sync()
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    parents, thres = [], []
    for j in range(2):                       # a parent: the assembly with its own substitutions, sequenced at 30x
        gen = torch.Generator(device=dev).manual_seed(7700 + j)
        g = d_asm.clone()
        hit = (torch.rand(g.numel(), generator=gen, device=dev) < SNP) & (g != ord("N"))
        shift = torch.randint(1, 4, (int(hit.sum().item()),), generator=gen, device=dev)
        g[hit] = lut[(code[g[hit].long()] + shift) % 4]
        pr = synth.torch_reads_stream(gen, g, nreads, bench.READ_LEN, 0.003)
        torch.cuda.synchronize(dev)          # (the table counts on a stream of its own)
        t = KmerTable(bench.K, min_slots=slots)
        t.count_bases_device(pr.data_ptr(), pr.numel())
        t.sync()
        del pr, g
        parents.append(t)
        rows = t.histo_rows()
        txt = polisher.threshold_from_histo_rows(rows)[0]
        sys.stderr.write("parent %d: distinct %d, histogram head %s, threshold %r\n" % (j, t.info()["distinct"], rows[:12], txt))
        thres.append(int(txt) if txt.split() else thr)      # (no threshold from the histogram: the child's)
    m, p = parents
    text = [0, offs[-1]]
    head = {"mode": mode, "lib": os.environ.get("JASPER_AMD_LIB", ""), "k": bench.K, "bases": asm_len, "thr": thr, "thr_mat": thres[0], "thr_pat": thres[1], "peak": peak,
            "r_slots": r.info()["slots"], "m_slots": m.info()["slots"], "m_distinct": m.info()["distinct"], "a_slots": a.info()["slots"]}
    scan = lambda: r.hapmer_scan_device(m, p, d_asm, text, thres[0], thres[1], thr)
    if mode == "trace":
        for _ in range(2):
            cr = r.copy_report_device(a, d_asm, text, thr, peak)
        for _ in range(2):
            sp = r.spectrum(a)
        for _ in range(2):
            hs = scan()
        for _ in range(2):
            cen = r.hapmer_census(m, p, a, thres[0], thres[1], thr)
        head.update({"copyrep_seconds": cr.seconds, "spectrum_seconds": sp.seconds, "hapscan_seconds": hs.seconds, "census_seconds": cen.seconds})
    else:
        secs, wall, csecs, cens, specs = [], [], [], [], []
        for _ in range(6):
            t0 = time.perf_counter()
            hs = scan()
            wall.append(time.perf_counter() - t0)
            secs.append(hs.seconds)
        for _ in range(6):
            csecs.append(r.copy_report_device(a, d_asm, text, thr, peak).seconds)
        for _ in range(3):
            cen = r.hapmer_census(m, p, a, thres[0], thres[1], thr)
            cens.append(cen.seconds)
            specs.append(r.spectrum(a).seconds)
        head.update({"hapscan_seconds": secs[1:], "wall_seconds": wall[1:], "copyrep_seconds": csecs[1:], "ratio_of_medians": sorted(secs[1:])[2] / sorted(csecs[1:])[2],
                     "census_seconds": cens[1:], "spectrum_seconds": specs[1:]})
    tot = [sum(c[i] for c in hs.counts) for i in range(4)]
    head.update({"counts": tot, "candidate_share": (tot[2] + tot[3]) / max(tot[1], 1), "runs": len(hs.runs), "retried": hs.retried, "census_mat": cen.mat, "census_pat": cen.pat,
                 "occurrences_equal_windows": [cen.mat[2] == tot[2], cen.pat[2] == tot[3]]})
    print(json.dumps(head))
    for t in (a, m, p, r):
        t.close()


if __name__ == "__main__":
    main()
