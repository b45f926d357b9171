"""The select (table_select_kernel, csrc/select.hip) next to the census it materialises, and read_bins on the marker tables next to
read_bins on the parental tables, on the workload of tools/prof_readbins.py (47 Mb synthetic genome, two synthetic
parents 0.1 % away, 30x of 150-base reads, k = 37).  Every number is the calls' own HIP-event seconds.

    python tools/prof_select.py time      (run on the GPU box)

  (a) KmerTable.select(M, P, None, tm, 1) and its mirror -- the two sweeps with the compaction, without the imports -- next to
      KmerTable.hapmer_census_parents(M, P, None, tm, tp): the same reads of M and P without the compaction.  The selects' wall
      seconds (sweep + import + fit) are given beside them
  (b) KmerTable.read_bins_device(M', P', batch, 1, 1) next to KmerTable.read_bins_device(M, P, batch, tm, tp), the path without
      --marker-tables, on the first 256 Mi bases of the child's reads; and that both give the same counts read by read
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode != "time":
        sys.exit(__doc__)
    import numpy as np
    import torch
    import bench
    import prof_readbins
    from jasper_amd import KmerTable
    dev = torch.device("cuda", 0)
    reads, nreads, m, p, tm, tp = prof_readbins.workload(torch, dev)
    rl = bench.READ_LEN
    head = {"mode": mode, "k": bench.K, "reads": nreads, "thr_mat": tm, "thr_pat": tp, "m_slots": m.info()["slots"], "m_distinct": m.info()["distinct"],
            "p_slots": p.info()["slots"], "p_distinct": p.info()["distinct"]}
    # (a) the selects next to the census
    census = [KmerTable.hapmer_census_parents(m, p, None, tm, tp) for _ in range(6)][1:]
    sel, walls, tables = [], [], None
    for _ in range(6):
        if tables:
            for t in tables:
                t.close()
        t0 = time.perf_counter()
        mm, sm = KmerTable.select(m, p, None, tm, 1)
        pp, sp = KmerTable.select(p, m, None, tp, 1)
        walls.append(time.perf_counter() - t0)
        sel.append(sm["seconds"] + sp["seconds"])
        tables = (mm, pp)
    mm, pp = tables
    head.update({"census_seconds": [c.seconds for c in census], "select_seconds": sel[1:], "select_wall_seconds": walls[1:],
                 "census_median": median([c.seconds for c in census]), "select_median": median(sel[1:]), "select_wall_median": median(walls[1:]),
                 "select_over_census": median(sel[1:]) / median([c.seconds for c in census]),
                 "mat": {k: v for k, v in sm.items() if k != "seconds"}, "pat": {k: v for k, v in sp.items() if k != "seconds"},
                 "equal_to_census": bool(census[-1].mat[0] == sm["selected"] and census[-1].pat[0] == sp["selected"]),
                 "marker_slots": [mm.info()["slots"], pp.info()["slots"]]})
    # (b) read_bins on the marker tables next to read_bins on the parents
    n = min(nreads, prof_readbins.BATCH_BASES // rl)
    text = reads.view(-1, rl + 1)[:n, :rl].contiguous()
    del reads
    torch.cuda.synchronize(dev)
    offs = np.arange(n + 1, dtype=np.int64) * rl
    old = [KmerTable.read_bins_device(m, p, text, offs, tm, tp) for _ in range(6)]
    new = [KmerTable.read_bins_device(mm, pp, text, offs, 1, 1) for _ in range(6)]
    so, sn = [r.seconds for r in old[1:]], [r.seconds for r in new[1:]]
    head.update({"batch_reads": n, "batch_bases": n * rl, "read_bins_parents_seconds": so, "read_bins_markers_seconds": sn, "read_bins_parents_median": median(so),
                 "read_bins_markers_median": median(sn), "markers_over_parents": median(sn) / median(so),
                 "equal_counts": bool((old[-1].mat == new[-1].mat).all() and (old[-1].pat == new[-1].pat).all())})
    print(json.dumps(head))
    for t in (m, p, mm, pp):
        t.close()


if __name__ == "__main__":
    main()
