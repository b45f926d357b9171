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
    if mode == "gz":
        return gz_e2e(torch, reads, nreads, m, p, tm, tp, head)
    if mode == "wgz":
        return wgz_e2e(torch, reads, nreads, m, p, tm, tp, head)
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


def _deflate_piece(args):
    import zlib
    data, last = args
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH)


def write_gz(path, buf, procs=16):
    """buf (np.uint8) as ONE gzip member at level 6; the pieces are deflated side by side and joined at full flushes, as pigz joins them"""
    import struct
    from multiprocessing.pool import ThreadPool         # (zlib releases the interpreter lock: threads deflate side by side, and nothing is forked beside the GPU runtime)
    import zlib
    step = -(-len(buf) // (4 * procs))
    pieces = [(buf[i:i + step].tobytes(), i + step >= len(buf)) for i in range(0, len(buf), step)]
    with ThreadPool(procs) as pool, open(path, "wb") as f:
        f.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03")
        for part in pool.imap(_deflate_piece, pieces):
            f.write(part)
        f.write(struct.pack("<II", zlib.crc32(buf), len(buf) & 0xFFFFFFFF))


def route_block(torch, m, text, rec_len, head):
    """the route kernels on one 64 MiB block of the file's text: medians of five after a warm-up, next to a device-to-device copy of the
    same bytes and to the three numpy mask gathers the host second pass does"""
    import numpy as np
    n = 64 << 20
    buf = text[:n]
    starts = np.arange(0, n, rec_len, dtype=np.int64)
    bounds = np.append(starts, n)
    codes = np.random.default_rng(5).integers(0, 3, len(starts)).astype(np.uint8)
    out = [np.empty(n, dtype=np.uint8) for _ in range(3)]
    secs = [m.route_text(buf, bounds, codes, b"@", 0, out).seconds for _ in range(6)][1:]
    d = torch.frombuffer(bytearray(buf.tobytes()), dtype=torch.uint8).cuda()
    e = torch.empty_like(d)
    copies = []
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.copy_(d)
        b.record()
        torch.cuda.synchronize()
        copies.append(a.elapsed_time(b) * 1e-3)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        size = np.diff(bounds)
        parts = [buf[np.repeat(codes == b, size)] for b in range(3)]
        host.append(time.perf_counter() - t0)
    r = m.route_text(buf, bounds, codes, b"@", 0, out)
    head["route_block"] = {"bytes": n, "segments": len(starts), "route_kernel_seconds": secs, "route_median": sorted(secs)[2], "d2d_copy_seconds": copies[1:],
                           "d2d_median": sorted(copies[1:])[2], "numpy_mask_seconds": host, "equal_to_numpy": all(r.out[b].tobytes() == parts[b].tobytes() for b in range(3))}
    del d, e


def gz_e2e(torch, reads, nreads, m, p, tm, tp, head):
    """the tool end to end on the workload as one level-6 .fastq.gz: --gz host / device without --write-reads, and the four --gz x --route
    settings with it, two runs each, alternating, in the order run; then the route kernels on one block"""
    import numpy as np
    import bench
    rl = bench.READ_LEN
    d = os.environ.get("TMPDIR", "/tmp")
    paths = {w: os.path.join(d, "prof_readbins_%s" % w) for w in ("mat.jf", "pat.jf", "child.fq.gz", "out")}
    m.write_jf(paths["mat.jf"])
    p.write_jf(paths["pat.jf"])
    seq = reads.view(-1, rl + 1)[:, :rl].cpu().numpy()
    del reads
    torch.cuda.empty_cache()
    rec = np.empty((nreads, 3 + rl + 3 + rl + 1), dtype=np.uint8)      # @r \n seq \n + \n qual \n
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + rl] = seq
    rec[:, 3 + rl:6 + rl] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + rl:6 + 2 * rl] = ord("I")
    rec[:, -1] = 10
    del seq
    text = rec.reshape(-1)
    route_block(torch, m, text, rec.shape[1], head)     # (in this process: if it faults, the process ends here and no child is ever started)
    m.close()
    p.close()
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    write_gz(paths["child.fq.gz"], text)
    head.update({"text_bytes": int(text.size), "gz_bytes": os.path.getsize(paths["child.fq.gz"]), "gz_write_seconds": time.perf_counter() - t0})
    del rec, text
    print(json.dumps(head), flush=True)
    args = ["-r", paths["child.fq.gz"], "--mat-jf", paths["mat.jf"], "--pat-jf", paths["pat.jf"], "--mat-threshold", str(tm), "--pat-threshold", str(tp), "-o", paths["out"],
            "--reader", "device"]
    plain = [["--gz", "host"], ["--gz", "device"]]
    written = [["--write-reads", "--gz", g, "--route", r] for g in ("host", "device") for r in ("host", "device")]
    runs = [(ROOT, f) for f in ((plain + written) if "quick" in sys.argv[2:] else (plain + plain + written + written))]
    parent = [a[len("parent="):] for a in sys.argv[2:] if a.startswith("parent=")]
    if parent:                                          # a built copy of the parent commit's tree: its tool knows neither flag and does what host / host does
        runs += [(os.path.abspath(parent[0]), ["--write-reads"]), (ROOT, ["--write-reads", "--gz", "host", "--route", "host"])]
    sums = {}
    # one child at a time, each under a time limit of its own; the first that fails, is killed by a signal or runs out of time ends the
    # run -- nothing more is started on the GPU after it, and what was collected up to then is already written
    for tree, flags in runs:
        limit = 240 if "host" in flags[-3:] or flags == ["--write-reads"] else 150
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, "-m", "jasper_amd.triobin"] + args + flags, env=dict(os.environ, PYTHONPATH=tree, JASPER_AMD_TIMING="1"), capture_output=True,
                               text=True, timeout=limit, cwd=tree)
            rc, err = r.returncode, r.stderr
        except subprocess.TimeoutExpired as e:
            rc, err = 124, (e.stderr or b"").decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        wall = time.perf_counter() - t0
        lines = [ln for ln in err.splitlines() if ln.startswith("[triobin]")]
        digest = None
        if rc == 0 and "--write-reads" in flags:
            import hashlib
            digest = {}
            for b in ("mat", "pat", "unknown"):
                fn = "%s.%s.prof_readbins_child.fq" % (paths["out"], b)
                h = hashlib.sha256()
                with open(fn, "rb") as f:
                    for blk in iter(lambda: f.read(1 << 24), b""):
                        h.update(blk)
                digest[b] = h.hexdigest()[:16]
                os.remove(fn)
            sums.setdefault("read_files", digest)
        table = open(paths["out"] + ".readbins.tsv").read() if rc == 0 else None
        sums.setdefault("table", table)
        print(json.dumps({"tree": "this commit" if tree == ROOT else "parent commit", "flags": flags, "returncode": rc, "time_limit": limit, "wall_seconds": wall, "lines": lines,
                          "same_table": table == sums["table"], "same_read_files": digest == sums.get("read_files") if digest else None,
                          "stderr_tail": err[-400:] if rc else None}), flush=True)
        if rc != 0:
            break
    for fn in list(paths.values()) + [paths["out"] + ".readbins.tsv"]:
        if os.path.exists(fn):
            os.remove(fn)


def deflate_block(torch, m, text, head):
    """the compressor on 64 MiB of the file's text: five timed calls after a warm-up (HIP events), next to a device-to-device copy of the
    same bytes; its size next to the host compressor's (zlib level 1, the same blocking, one core, timed) and zlib level 6 over the block"""
    import zlib
    import numpy as np
    from jasper_amd import bgzf
    n = 64 << 20
    buf = text[:n]
    out = np.empty(n + 31 * (-(-n // bgzf.BLOCK)), dtype=np.uint8)
    got = [m.deflate_bgzf(buf, out=out) for _ in range(6)]
    secs = [g[2] for g in got[1:]]
    members = got[-1][0]
    d = torch.frombuffer(bytearray(buf.tobytes()), dtype=torch.uint8).cuda()
    e = torch.empty_like(d)
    copies = []
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.copy_(d)
        b.record()
        torch.cuda.synchronize()
        copies.append(a.elapsed_time(b) * 1e-3)
    del d, e
    t0 = time.perf_counter()
    host = bgzf.compress(buf)
    host_secs = time.perf_counter() - t0
    t0 = time.perf_counter()
    six = len(zlib.compress(buf, 6))
    six_secs = time.perf_counter() - t0
    import gzip
    head["deflate_block"] = {"bytes": n, "deflate_kernel_seconds": secs, "deflate_median": sorted(secs)[2], "d2d_copy_seconds": copies[1:], "d2d_median": sorted(copies[1:])[2],
                             "counters": got[-1][1], "device_bytes": int(len(members)), "host_level1_bgzf_bytes": len(host), "host_level1_bgzf_seconds": host_secs,
                             "zlib_level6_bytes": six, "zlib_level6_seconds": six_secs, "inflates_to_the_text": gzip.decompress(members.tobytes()) == buf.tobytes()}


def wgz_e2e(torch, reads, nreads, m, p, tm, tp, head):
    """`--write-gz` end to end on the workload as one level-6 .fastq.gz, every device flag on: --deflate device twice; the plain run (what
    the parent commit writes) and `gzip -1` of its three files on one core, which is what a user does without the flag; --deflate host.
    Every .gz file's text is held to the plain run's by SHA-256 (gzip -dc).  Then nothing else is started."""
    import hashlib
    import numpy as np
    import bench
    rl = bench.READ_LEN
    d = os.environ.get("TMPDIR", "/tmp")
    paths = {w: os.path.join(d, "prof_readbins_%s" % w) for w in ("mat.jf", "pat.jf", "child.fq.gz", "out")}
    m.write_jf(paths["mat.jf"])
    p.write_jf(paths["pat.jf"])
    seq = reads.view(-1, rl + 1)[:, :rl].cpu().numpy()
    del reads
    torch.cuda.empty_cache()
    rec = np.empty((nreads, 3 + rl + 3 + rl + 1), dtype=np.uint8)      # @r \n seq \n + \n qual \n
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + rl] = seq
    rec[:, 3 + rl:6 + rl] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + rl:6 + 2 * rl] = ord("I")
    rec[:, -1] = 10
    del seq
    text = rec.reshape(-1)
    deflate_block(torch, m, text, head)                 # (in this process: if it faults, the process ends here and no child is ever started)
    m.close()
    p.close()
    torch.cuda.empty_cache()
    write_gz(paths["child.fq.gz"], text)
    head.update({"text_bytes": int(text.size), "gz_bytes": os.path.getsize(paths["child.fq.gz"])})
    del rec, text
    print(json.dumps(head), flush=True)
    args = ["-r", paths["child.fq.gz"], "--mat-jf", paths["mat.jf"], "--pat-jf", paths["pat.jf"], "--mat-threshold", str(tm), "--pat-threshold", str(tp), "-o", paths["out"],
            "--reader", "device", "--gz", "device", "--route", "device", "--write-reads"]
    dev = ["--write-gz", "--deflate", "device"]
    runs = [dev, dev, [], ["--write-gz", "--deflate", "host"]]
    names = ["%s.%s.prof_readbins_child.fq" % (paths["out"], b) for b in ("mat", "pat", "unknown")]

    def sha(cmd):
        h = hashlib.sha256()
        with subprocess.Popen(cmd, stdout=subprocess.PIPE) as pr:
            for blk in iter(lambda: pr.stdout.read(1 << 24), b""):
                h.update(blk)
        return h.hexdigest()[:16] if pr.returncode == 0 else None

    want = None
    for i, flags in enumerate(runs):
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, "-m", "jasper_amd.triobin"] + args + flags, env=dict(os.environ, PYTHONPATH=ROOT, JASPER_AMD_TIMING="1"), capture_output=True,
                               text=True, timeout=400, cwd=ROOT)
            rc, err = r.returncode, r.stderr
        except subprocess.TimeoutExpired:
            rc, err = 124, ""
        wall = time.perf_counter() - t0
        line = {"flags": flags, "returncode": rc, "wall_seconds": wall, "lines": [ln for ln in err.splitlines() if ln.startswith("[triobin]")], "stderr_tail": err[-400:] if rc else None}
        if rc == 0 and not flags:                       # the plain files: their digests, then what a user does with them today
            want = [sha(["cat", fn]) for fn in names]
            line["plain_bytes"] = [os.path.getsize(fn) for fn in names]
            t0 = time.perf_counter()
            sizes = []
            for fn in names:
                with open(fn + ".1.gz", "wb") as f:
                    subprocess.check_call(["gzip", "-1", "-c", fn], stdout=f)
                sizes.append(os.path.getsize(fn + ".1.gz"))
                os.remove(fn + ".1.gz")
            line.update({"gzip_1_one_core_seconds": time.perf_counter() - t0, "gzip_1_bytes": sizes})
            t0 = time.perf_counter()
            with open(names[0], "rb") as f:
                sample = f.read(256 << 20)
            pr = subprocess.run(["gzip", "-6", "-c"], input=sample, stdout=subprocess.PIPE)
            line.update({"gzip_6_sample_bytes": len(sample), "gzip_6_sample_out": len(pr.stdout), "gzip_6_sample_seconds": time.perf_counter() - t0})
            del sample, pr
        elif rc == 0:
            line["gz_bytes"] = [os.path.getsize(fn + ".gz") for fn in names]
            if i != 0:                                  # (the first device run's files are checked after the plain run has given the digests)
                line["same_text_as_plain"] = [sha(["gzip", "-dc", fn + ".gz"]) for fn in names] == want if want else None
        if i == 0 and rc == 0:
            keep = [fn + ".gz.first" for fn in names]
            for fn, k in zip(names, keep):
                os.replace(fn + ".gz", k)
        print(json.dumps(line), flush=True)
        if rc != 0:
            break
    else:
        print(json.dumps({"first_device_run_same_text_as_plain": [sha(["gzip", "-dc", fn + ".gz.first"]) for fn in names] == want}), flush=True)
    for fn in list(paths.values()) + [paths["out"] + ".readbins.tsv"] + names + [fn + ".gz" for fn in names] + [fn + ".gz.first" for fn in names]:
        if os.path.exists(fn):
            os.remove(fn)


if __name__ == "__main__":
    main()
