"""What the gap scan costs, on bench.py's workload (47 Mb synthetic assembly, 30x reads, k = 37) with about 1 000 planted gaps.

    python tools/prof_gaps.py       (run on the GPU box; tools/prof_gaps.sh keeps its output)

R = the counted read table, the threshold = 2 (DESIGN 4.9's), the text = the unpolished assembly as ONE sequence in which, about every
47 kb, 100 to 2 000 bases are taken out and 100 Ns put in.  No profiler: the library's own event times.  Prints one JSON line with
  the dense half    report_seconds (report_scan_kernel and its stitch kernels) next to runs_seconds (gap_runs_kernel and its)
  the search        at --gap-max-len 1000 and 4096: search_seconds of three scans after a warm-up, lookups, the nine counters, and how
                    many of the planted gaps come back unique and equal to the truth -- the bases that were taken out or, where the
                    assembly had an error among them, a string that the genome holds between the same flanks
  the yardstick     compound_search_kernel on the same text at max_len 64: its seconds, sites and lookups
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_GAPS, N_RUN, SEED = 1000, 100, 2


def plant(asm, rng):
    """(text, [(a, bases taken out)]): a = where the N run starts in the text"""
    import numpy as np
    step = len(asm) // (N_GAPS + 1)
    pieces, plants, last, shift = [], [], 0, 0
    for i in range(1, N_GAPS + 1):
        p = i * step + int(rng.integers(0, step // 4))
        took = int(rng.integers(100, 2001))
        if ord("N") in asm[p - 100:p + took + 100]:          # (the assembly's own gaps stay as they are)
            continue
        pieces += [asm[last:p], np.full(N_RUN, ord("N"), dtype=np.uint8)]
        plants.append((p + shift, asm[p:p + took].tobytes()))
        shift += N_RUN - took
        last = p + took
    pieces.append(asm[last:])
    return np.concatenate(pieces), plants


def main():
    import numpy as np
    import torch
    import bench
    from jasper_amd import KmerTable, synth
    dev = torch.device("cuda", 0)
    reads, names, seqs, (d_asm, offs), asm_len, bs, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, SEED)
    genome = synth.torch_genome(torch.Generator(device=dev).manual_seed(SEED * 1000), int(47.0 * 1e6), dev).cpu().numpy().tobytes()
    r = KmerTable(bench.K, min_slots=max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10)))      # (sized as bench.py sizes it)
    r.count_bases_device(reads.data_ptr(), reads.numel())
    r.sync()
    del reads
    thr = 2
    text, plants = plant(d_asm.cpu().numpy(), np.random.default_rng(SEED))
    d_text = torch.from_numpy(text).to(dev)
    torch.cuda.synchronize(dev)
    host = text.tobytes()
    offs1 = [0, len(text)]
    out = {"k": bench.K, "bases": len(text), "thr": thr, "planted": len(plants)}
    for max_len in (1000, 4096):
        secs = []
        for _ in range(4):
            gs = r.gap_scan_device(d_text, offs1, thr, max_len)
            secs.append(gs.search_seconds)
        fills = {(int(s["a"])): None for s in gs.sites if int(s["n_records"]) == 1 and int(s["status"]) != 3}
        for rec in gs.records:
            if int(rec["pos"]) in fills:
                fills[int(rec["pos"])] = (int(rec["ref_len"]), gs.fill(rec).encode())
        exact = in_genome = within = 0
        for a, took in plants:
            within += len(took) <= max_len
            got = fills.get(a)
            if got is None:
                continue
            if got == (N_RUN, took):
                exact += 1
            elif genome.find(host[a - 40:a] + got[1] + host[a + got[0]:a + got[0] + 40]) >= 0:
                in_genome += 1
        out["max_len_%d" % max_len] = {"search_seconds": secs[1:], "lookups": gs.lookups, "retried": gs.retried, "counts": list(gs.counts[0]),
                                       "planted_within_max_len": within, "unique_and_equal_to_what_was_taken_out": exact, "unique_and_in_the_genome_between_the_flanks": in_genome,
                                       "report_seconds": gs.report.seconds, "runs_seconds": gs.runs_seconds}
    cs_secs = []
    for _ in range(4):
        cs = r.compound_scan_device(d_text, offs1, thr, 64)
        cs_secs.append(cs.search_seconds)
    out["compound_64"] = {"search_seconds": cs_secs[1:], "lookups": cs.lookups, "counts": list(cs.counts[0])}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
