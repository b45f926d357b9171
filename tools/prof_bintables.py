"""The two kernels of `triobin --write-jf` next to their yardsticks, on bench.py's workload with reads (47 Mb synthetic genome, 30x of
150-base reads, k = 37): DESIGN 4.18's numbers.

    python tools/prof_bintables.py time [GENOME_MB]      (run on the GPU box; writes three JSON lines)

The batch = the first 256 Mi bases of the reads, packed back to back without separators (what one call of the tool sends), with bin
codes drawn 20 % / 20 % / 60 % (hap1 / hap2 / unknown).
  gather    KmerTable.count_binned_device with ONE sink that takes every read: reads_gather_kernel's own event seconds for all of the
            batch's bytes, next to a device-to-device copy of the same bytes (torch, events; five of each after a warm-up).  The sink's
            table is R; its counting seconds are the call's
  bins      the same call with the two sinks {0} and {1}: T1 and T2, a fifth of the bytes each
  subtract  KmerTable.subtract(R, T2) next to R.spectrum(T2) (the spectrum's sweep over the same table, one probe as well) and
            KmerTable.select(R, T2, T1) (two probes); three of each after a warm-up, and the subtract's five counters
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH_BASES = 256 << 20


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    import numpy as np
    import torch
    import bench
    from jasper_amd import KmerTable
    genome_mb = float(sys.argv[2]) if len(sys.argv) > 2 else 47.0
    dev = torch.device("cuda", 0)
    reads, _, _, _, _, _, nreads = bench.build_workload(torch, dev, 0, 1, genome_mb, 2)
    rl = bench.READ_LEN
    n = min(nreads, BATCH_BASES // rl)
    text = reads.view(-1, rl + 1)[:n, :rl].contiguous()
    del reads
    torch.cuda.synchronize(dev)
    offs = np.arange(n + 1, dtype=np.int64) * rl
    codes = np.random.default_rng(5).choice(np.array([0, 1, 2], dtype=np.uint8), size=n, p=[0.2, 0.2, 0.6])
    out = {"k": bench.K, "genome_mb": genome_mb, "batch_reads": n, "batch_bases": n * rl}
    slots = max(1 << 21, int(1.25 * n * rl * 2.1 / 10))

    # the gather over every byte, and the copy of the same bytes
    gather, counting = [], []
    r_table = None
    for rep in range(6):
        if r_table is not None:
            r_table.close()
        r_table = KmerTable(bench.K, min_slots=slots)
        st = KmerTable.count_binned_device(text, offs, codes, [(r_table, (0, 1, 2))])[0]
        gather.append(st["gather_seconds"])
        counting.append(st["count_seconds"])
    moved = st["bases"] + st["reads"]
    dst = torch.empty(moved, dtype=torch.uint8, device=dev)
    src = torch.empty(moved, dtype=torch.uint8, device=dev)
    copies = []
    for rep in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize(dev)
        copies.append(e0.elapsed_time(e1) * 1e-3)
    del dst, src
    g, c = median(gather[1:]), median(copies[1:])
    out["gather"] = {"bytes": moved, "seconds": gather[1:], "median": g, "bytes_per_second": moved / g, "copy_seconds": copies[1:], "copy_median": c,
                     "copy_bytes_per_second": moved / c, "gather_over_copy": g / c, "count_seconds": counting[1:], "r_distinct": r_table.info()["distinct"],
                     "r_slots": r_table.info()["slots"]}

    # the two bins
    t1, t2 = KmerTable(bench.K, min_slots=slots // 4), KmerTable(bench.K, min_slots=slots // 4)
    st = KmerTable.count_binned_device(text, offs, codes, [(t1, (0,)), (t2, (1,))])
    out["bins"] = [{key: s[key] for key in ("reads", "bases", "occurrences", "gather_seconds", "count_seconds")} for s in st]
    out["bins_distinct"] = [t1.info()["distinct"], t2.info()["distinct"]]
    del text

    # the subtract and its yardsticks (a yardstick that fails leaves its message in place of its seconds: a select that keeps most
    # of R's keys outgrows the marker-sized table KmerTable.select starts from)
    print(json.dumps(out), flush=True)
    sub, sel2, spec = [], [], []
    for rep in range(4):
        d, s = KmerTable.subtract(r_table, t2)
        sub.append(s["seconds"])
        counters = {key: s[key] for key in ("swept", "matched", "dropped", "underflow", "kept", "missing")}
        d.close()
        spec.append(r_table.spectrum(t2).seconds)
    out = {"subtract": {"seconds": sub[1:], "median": median(sub[1:]), "slots_per_second": r_table.info()["slots"] / median(sub[1:]), "counters": counters,
                        "spectrum": spec[1:], "over_spectrum": median(sub[1:]) / median(spec[1:])}}
    print(json.dumps(out), flush=True)
    try:
        for rep in range(4):
            d, s = KmerTable.select(r_table, t2, t1)
            sel2.append(s["seconds"])
            d.close()
        out = {"select_two_probes": sel2[1:], "subtract_over_select_two_probes": median(sub[1:]) / median(sel2[1:])}
    except Exception as e:      # noqa: BLE001
        out = {"select_two_probes": str(e), "seconds_before_it_failed": sel2}
    for t in (r_table, t1, t2):
        t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "time":
        sys.exit(__doc__)
    main()
