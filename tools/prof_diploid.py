"""The pair spectrum and the pair scan next to what a user could run before them, on bench.py's workload (47 Mb synthetic assembly, 30x
reads, k = 37) with a second haplotype 0.1 % away (substitutions).

    python tools/prof_diploid.py time       (run on the GPU box)

R = the counted read table, A1 = the assembly counted into a table of its own, A2 = the second haplotype counted into another, the text =
the assembly as ONE sequence in host memory.  All in one process, no profiler; five timed calls after a warm-up call of the same kind,
device seconds by HIP events (what the results carry):
  join   spectrum(R, A1) and spectrum(R, A2), both untouched by the pair spectrum, against spectrum_pair(R, A1, A2): R swept twice against once
  scan   copy_report(R, A2, text) against pair_scan(R, A2, text): the same text, the same two tables, two probes per window each
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode != "time":
        sys.exit(__doc__)
    import numpy as np
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
    text = b"".join(seqs)
    a1 = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    a1.count_bases(text)
    # the second haplotype: one base in a thousand replaced by another one
    rng = np.random.default_rng(2)
    hap = np.frombuffer(text, dtype=np.uint8).copy()
    pos = rng.choice(len(hap), size=len(hap) // 1000, replace=False)
    pos = pos[np.isin(hap[pos], np.frombuffer(b"ACGT", dtype=np.uint8))]
    code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), hap[pos])
    hap[pos] = np.frombuffer(b"ACGT", dtype=np.uint8)[(code + rng.integers(1, 4, len(pos))) % 4]
    a2 = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    a2.count_bases(hap.tobytes())
    del hap
    ri, i1, i2 = r.info(), a1.info(), a2.info()
    head = {"mode": mode, "k": bench.K, "bases": asm_len, "thr": thr, "peak": peak, "substitutions": int(len(pos)), "r_slots": ri["slots"], "r_distinct": ri["distinct"],
            "a1_slots": i1["slots"], "a1_distinct": i1["distinct"], "a2_slots": i2["slots"], "a2_distinct": i2["distinct"]}
    s1, s2, sp, wall = [], [], [], []
    for _ in range(6):
        s1.append(r.spectrum(a1).seconds)
        s2.append(r.spectrum(a2).seconds)
        t0 = time.perf_counter()
        pair = r.spectrum_pair(a1, a2)
        wall.append(time.perf_counter() - t0)
        sp.append(pair.seconds)
    head.update({"spectrum_a1_seconds": s1[1:], "spectrum_a2_seconds": s2[1:], "spectrum_pair_seconds": sp[1:], "spectrum_pair_wall_seconds": wall[1:],
                 "join_ratio_of_medians": median(sp[1:]) / (median(s1[1:]) + median(s2[1:])), "pair_row_sums": [int(x) for x in pair.cells.sum(axis=1)]})
    cs, ps = [], []
    for _ in range(6):
        cs.append(r.copy_report(a2, [text], thr, peak).seconds)
        scan = r.pair_scan(a2, [text], thr)
        ps.append(scan.seconds)
    head.update({"copyrep_seconds": cs[1:], "pairscan_seconds": ps[1:], "scan_ratio_of_medians": median(ps[1:]) / median(cs[1:]), "pairscan_counts": scan.counts[0],
                 "pairscan_runs": len(scan.runs), "retried": scan.retried})
    print(json.dumps(head))
    for t in (a1, a2, r):
        t.close()


if __name__ == "__main__":
    main()
