"""The duplication map's two kernels next to their yardstick, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37) with
duplicated segments planted into the assembly.

    python tools/prof_dups.py time       (run on the GPU box, no profiler; tools/prof_dups.sh keeps the output)

R = the counted read table, the text = the assembly as ONE sequence with PLANT_N segments of PLANT_LEN bases each copied to another place
(every second one reverse-complemented): 2 * PLANT_N * PLANT_LEN bases lie in a two-copy stretch.  A = that text counted into a table of
its own.  Threshold 2.  HIP events, medians of five calls after a warm-up, all in one process:
  copies_scan_kernel + the stitch kernels (jasper_copyrep_seconds): the yardstick, two probes per window
  dup_index_kernel + the side array's fill (jasper_dupmap_seconds, index): one probe per window, two atomics per count-2 window
  dup_scan_kernel + the stitch kernels (jasper_dupmap_seconds, scan): two probes per window, one 16-byte load per count-2 window
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANT_N, PLANT_LEN, THRE = 40, 50_000, 2


def plant(torch, d_asm, n):
    """PLANT_N segments copied within the text, sources in the first half and targets in the second, evenly spread"""
    comp = torch.arange(256, dtype=torch.uint8, device=d_asm.device)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    half = n // 2
    step = (half - PLANT_LEN) // PLANT_N
    for i in range(PLANT_N):
        src, dst = i * step, half + i * step
        seg = d_asm[src:src + PLANT_LEN].clone()
        d_asm[dst:dst + PLANT_LEN] = comp[seg.long()].flip(0) if i & 1 else seg
    return 2 * PLANT_N * PLANT_LEN


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    import bench
    from jasper_amd import KmerTable, copies
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    n = int(offs[-1])
    planted = plant(torch, d_asm, n)
    torch.cuda.synchronize()
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    peak = copies.peak_from_histogram(r.histogram(), THRE)
    a = KmerTable(bench.K, min_slots=max(1 << 16, int(1.25 * asm_len)))
    a.count_bases_device(d_asm.data_ptr(), n)
    a.sync()
    ri, ai = r.info(), a.info()
    text = [0, n]
    head = {"lib": os.environ.get("JASPER_AMD_LIB", ""), "k": bench.K, "bases": n, "planted_bases": planted, "thr": THRE, "peak": peak, "r_slots": ri["slots"],
            "r_distinct": ri["distinct"], "a_slots": ai["slots"], "a_distinct": ai["distinct"]}
    csecs, isecs, ssecs, wall = [], [], [], []
    for _ in range(6):
        csecs.append(r.copy_report_device(a, d_asm, text, THRE, peak).seconds)
    for _ in range(6):
        t0 = time.perf_counter()
        dm = r.dup_map_device(a, d_asm, text, THRE, peak)
        wall.append(time.perf_counter() - t0)
        isecs.append(dm.seconds[0])
        ssecs.append(dm.seconds[1])
    head.update({"copyrep_seconds": csecs[1:], "dup_index_seconds": isecs[1:], "dup_scan_seconds": ssecs[1:], "dup_wall_seconds": wall[1:],
                 "median_copyrep": median(csecs[1:]), "median_dup_index": median(isecs[1:]), "median_dup_scan": median(ssecs[1:]),
                 "scan_over_copyrep": median(ssecs[1:]) / median(csecs[1:]), "index_over_copyrep": median(isecs[1:]) / median(csecs[1:]),
                 "counts": dm.counts[0], "runs": len(dm.runs), "runs_of_1000_or_more": int((dm.runs["n_kmers"] >= 1000).sum()), "retried": dm.retried})
    print(json.dumps(head))
    a.close()
    r.close()


if __name__ == "__main__":
    main()
