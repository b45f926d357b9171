"""The read binning kernel next to its two yardsticks, on bench.py's workload with reads (47 Mb synthetic genome, two synthetic parents
0.1 % away, 30x of 150-base reads drawn from it, k = 37), and the tool's end-to-end time on the same reads.

    python tools/prof_readbins.py trace|time|e2e [--reader host|device]      (run on the GPU box; tools/prof_readbins.sh puts `trace` under rocprofv3)

M and P = each parent's reads at 30x, counted (as tools/prof_hapmers.py makes them).  The batch = the first 256 Mi bases of the child's
reads, packed back to back without separators: what one call of the tool sends.
  (a) hapmer_scan_kernel without a child over the batch's bytes as ONE contig: the same probes and no boundaries -- the ceiling
  (b) hapmer_scan_kernel without a child over the batch as separate sequences, one tile per read: what a user could do before
  (c) read_starts_kernel + read_bins_kernel over the batch
trace: each of the three after a warm-up call of the same kind, in one process so that one kernel trace holds them
time:  no profiler: the calls' own event seconds, five of (a) and (c) and three of (b) after a warm-up, and that (c) equals (b) read by read
e2e:   the parents written as databases and ALL the child's reads as one FASTQ file, then `python -m jasper_amd.triobin` as a child
       process on them: its wall seconds, the kernel's summed device seconds (JASPER_AMD_TIMING=1), and the seconds the tool's reader
       alone takes over the same file.  `--reader R` is passed on to the tool (with device its index + pack seconds are reported too)
summarize DIR: per kernel of a rocprofv3 --kernel-trace CSV under DIR the durations of its dispatches in order (the measured call's are
       the last ones)
"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SNP = 0.001
BATCH_BASES = 256 << 20


def summarize(d):
    out = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in sorted(csv.DictReader(open(fn)), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"].split("(")[0]
            if "read_bins" in name or "read_starts" in name or "hapmer_" in name or "scan_heads" in name or "scan_stitch" in name:
                out.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in sorted(out.items()):
        print(json.dumps({"kernel": name, "dispatches_us": [round(x, 1) for x in us]}))


def workload(torch, dev):
    """-> (the child's read stream in HBM, reads, M, P, thre_mat, thre_pat)"""
    import bench
    from jasper_amd import KmerTable, polisher, synth
    reads, _, _, (d_asm, offs), asm_len, _, nreads = bench.build_workload(torch, dev, 0, 1, 47.0, 2)
    slots = max(1 << 21, int(1.25 * nreads * bench.READ_LEN * 2.1 / 10))      # (sized as bench.py sizes the reads' table)
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
        txt = polisher.threshold_from_histo_rows(t.histo_rows())[0]
        thres.append(int(txt) if txt.split() else 2)
    del d_asm
    return reads, nreads, parents[0], parents[1], thres[0], thres[1]


def main():
    mode = sys.argv[1]
    if mode == "summarize":
        return summarize(sys.argv[2])
    import numpy as np
    import torch
    import bench
    from jasper_amd import KmerTable
    dev = torch.device("cuda", 0)
    reads, nreads, m, p, tm, tp = workload(torch, dev)
    rl = bench.READ_LEN
    head = {"mode": mode, "k": bench.K, "reads": nreads, "thr_mat": tm, "thr_pat": tp, "m_slots": m.info()["slots"], "m_distinct": m.info()["distinct"]}
    if mode == "e2e":
        return e2e(torch, reads, nreads, m, p, tm, tp, head)
    n = min(nreads, BATCH_BASES // rl)
    text = reads.view(-1, rl + 1)[:n, :rl].contiguous()      # the batch, packed: no separator bytes
    del reads
    torch.cuda.synchronize(dev)
    offs = np.arange(n + 1, dtype=np.int64) * rl
    head.update({"batch_reads": n, "batch_bases": n * rl})
    one = lambda: m.hapmer_scan_device(m, p, text, [0, n * rl], tm, tp, child=False)              # noqa: E731  (a)
    per = lambda: m.hapmer_scan_device(m, p, text, offs.tolist(), tm, tp, child=False)            # noqa: E731  (b)
    new = lambda: KmerTable.read_bins_device(m, p, text, offs, tm, tp)                             # noqa: E731  (c)
    if mode == "trace":
        for f in (one, per, new):
            for _ in range(2):
                r = f()
            head.setdefault("seconds", []).append(r.seconds)
    else:
        secs = {}
        for name, f, reps in (("a_one_contig", one, 6), ("b_per_read", per, 4), ("c_read_bins", new, 6)):
            got = [f() for _ in range(reps)]
            secs[name] = [g.seconds for g in got[1:]]
            if name == "b_per_read":
                b = got[-1]
            if name == "c_read_bins":
                c = got[-1]
        med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
        bm, bp = np.array([x[2] for x in b.counts], dtype=np.uint64), np.array([x[3] for x in b.counts], dtype=np.uint64)
        head.update({"seconds": secs, "median": med, "bases_per_second": {k: n * rl / v for k, v in med.items()}, "c_over_a": med["c_read_bins"] / med["a_one_contig"],
                     "b_over_c": med["b_per_read"] / med["c_read_bins"], "equal_to_b": bool((bm == c.mat).all() and (bp == c.pat).all()),
                     "marker_share": float((int(c.mat.sum()) + int(c.pat.sum())) / (n * (rl - bench.K + 1))), "reads_with_markers": int(((c.mat != 0) | (c.pat != 0)).sum())})
    print(json.dumps(head))
    m.close()
    p.close()


def e2e(torch, reads, nreads, m, p, tm, tp, head):
    import numpy as np
    import bench
    from jasper_amd import triobin
    rl = bench.READ_LEN
    d = os.environ.get("TMPDIR", "/tmp")
    paths = {w: os.path.join(d, "prof_readbins_%s" % w) for w in ("mat.jf", "pat.jf", "child.fq", "out")}
    m.write_jf(paths["mat.jf"])
    p.write_jf(paths["pat.jf"])
    m.close()
    p.close()
    seq = reads.view(-1, rl + 1)[:, :rl].cpu().numpy()
    del reads
    torch.cuda.empty_cache()
    rec = np.empty((nreads, 3 + rl + 3 + rl + 1), dtype=np.uint8)      # @r \n seq \n + \n qual \n
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + rl] = seq
    rec[:, 3 + rl:6 + rl] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + rl:6 + 2 * rl] = ord("I")
    rec[:, -1] = 10
    rec.tofile(paths["child.fq"])
    del rec, seq
    t0 = time.perf_counter()
    n = sum(len(ch.lens) for ch in triobin.chunks(paths["child.fq"]))
    reader = time.perf_counter() - t0
    assert n == nreads
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", paths["child.fq"], "--mat-jf", paths["mat.jf"], "--pat-jf", paths["pat.jf"], "--mat-threshold", str(tm),
                        "--pat-threshold", str(tp), "-o", paths["out"]] + sys.argv[2:], env=dict(os.environ, PYTHONPATH=ROOT, JASPER_AMD_TIMING="1"), capture_output=True, text=True)
    wall = time.perf_counter() - t0
    sys.stderr.write(r.stdout + r.stderr)
    dev_secs = re.search(r"read_bins device seconds: ([0-9.]+)", r.stderr)
    index_secs = re.search(r"read_text index \+ pack device seconds: ([0-9.]+)", r.stderr)
    head.update({"tool_flags": sys.argv[2:], "index_pack_device_seconds": float(index_secs.group(1)) if index_secs else None,
                 "returncode": r.returncode, "tool_wall_seconds": wall, "reader_alone_seconds": reader, "kernel_device_seconds": float(dev_secs.group(1)) if dev_secs else None,
                 "file_bytes": os.path.getsize(paths["child.fq"]), "table": open(paths["out"] + ".readbins.tsv").read() if r.returncode == 0 else None})
    print(json.dumps(head))
    for fn in list(paths.values()) + [paths["out"] + ".readbins.tsv"]:
        if os.path.exists(fn):
            os.remove(fn)


if __name__ == "__main__":
    main()
