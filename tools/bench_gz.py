#!/usr/bin/env python3
"""gzip read input: the device inflater (jasper_inflate_file_device, inflate_gpu.hip) against the host's many-thread reader
(jasper_inflate_file, pgunzip.hpp) on one single-member level-6 .fastq.gz of synthetic reads (jasper_amd.synth genome, 30x
150-bp reads, qualities drawn from a small alphabet so that the text compresses like real FASTQ).  Prints one JSON line:
inflate alone (text GB/s) and file -> table (s) for both engines, alternated and repeated, a size sweep for the crossover, and
whether the text and the histograms agree.

  python tools/bench_gz.py [--genome-mb 23.5] [--repeat 2] [--threads 16] [--sweep-mb 4,16,64,256]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

REC = 22 + 2 * 150 + 4   # bytes per FASTQ record of fastq()
PIECE = (8 << 20) // REC * REC   # text per independently compressed piece (whole records; the 32 KB before it as its dictionary)


def fastq(genome_mb, seed=3, coverage=30, rl=150):
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    g = synth.make_genome(rng, int(genome_mb * 1e6))
    n = int(len(g) * coverage / rl)
    hdr = b"@SIM:1:FCX:1:%08d\n"
    hl = len(hdr % 0)
    rec = np.empty((n, hl + 2 * rl + 4), dtype=np.uint8)
    ids = np.char.zfill(np.arange(n).astype("U8"), 8).astype("S8").view(np.uint8).reshape(n, 8)
    rec[:, :hl] = np.frombuffer(hdr % 0, dtype=np.uint8)
    rec[:, hl - 9:hl - 1] = ids
    bs = 1 << 20
    qa = np.frombuffer(b"FFFFFFFFF:,F#", dtype=np.uint8)
    for a in range(0, n, bs):
        m = min(bs, n - a)
        st = rng.integers(0, len(g) - rl + 1, m)
        rec[a:a + m, hl:hl + rl] = g[st[:, None] + np.arange(rl)]
        rec[a:a + m, hl + rl + 3:hl + 2 * rl + 3] = qa[rng.integers(0, len(qa), (m, rl))]
    rec[:, hl + rl] = ord("\n")
    rec[:, hl + rl + 1] = ord("+")
    rec[:, hl + rl + 2] = ord("\n")
    rec[:, -1] = ord("\n")
    return rec.tobytes()


def compress_pieces(text, threads):
    """level-6 raw deflate of every PIECE of text (sync-flushed, byte-aligned, non-final), in parallel: one gzip member is then
    header + the pieces in order + an empty final block + trailer (pigz's layout)"""
    def one(i):
        lo = i * PIECE
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, *([text[max(0, lo - 32768):lo]] if lo else []))
        return co.compress(text[lo:lo + PIECE]) + co.flush(zlib.Z_SYNC_FLUSH)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range((len(text) + PIECE - 1) // PIECE)))


def write_member(path, pieces, text, n_pieces):
    tlen = min(len(text), n_pieces * PIECE)
    crc = 0
    for lo in range(0, tlen, 1 << 28):
        crc = zlib.crc32(text[lo:min(tlen, lo + (1 << 28))], crc)
    with open(path, "wb") as f:
        f.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03")
        for p in pieces[:n_pieces]:
            f.write(p)
        f.write(b"\x03\x00")                                    # empty final fixed-Huffman block
        f.write((crc & 0xFFFFFFFF).to_bytes(4, "little") + (tlen & 0xFFFFFFFF).to_bytes(4, "little"))
    return tlen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=23.5, help="30x of it: 23.5 -> ~1.5 GB of FASTQ (the round-2 file's text)")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="host reader threads (a process on the GPU nodes gets 16 CPUs)")
    ap.add_argument("--sweep-mb", default="4,16,64,256", help="text MB of the sweep files (file -> table, both engines)")
    ap.add_argument("--k", type=int, default=37)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-table", action="store_true", help="inflate alone only (profiling runs)")
    a = ap.parse_args()
    from jasper_amd import _lib, KmerTable
    L = _lib.lib()
    d = a.dir or tempfile.mkdtemp(prefix="bench_gz_")
    t0 = time.perf_counter()
    text = fastq(a.genome_mb)
    pieces = compress_pieces(text, a.threads)
    path = os.path.join(d, "reads.fastq.gz")
    write_member(path, pieces, text, len(pieces))
    t_make = time.perf_counter() - t0
    zbytes = os.path.getsize(path)
    res = {"metric": "gzip_inflate", "text_bytes": len(text), "gz_bytes": zbytes, "host_threads": a.threads, "make_s": round(t_make, 1)}

    def host_inflate(p, out=None):
        n, par = C.c_uint64(0), C.c_int(0)
        t = time.perf_counter()
        rc = L.jasper_inflate_file(p.encode(), a.threads, 0, out.encode() if out else None, C.byref(n), C.byref(par))
        return time.perf_counter() - t, rc, n.value, par.value

    def dev_inflate(p, out=None):
        n, st = C.c_uint64(0), (C.c_uint64 * 6)()
        t = time.perf_counter()
        rc = L.jasper_inflate_file_device(0, p.encode(), 0, out.encode() if out else None, C.byref(n), st)
        return time.perf_counter() - t, rc, n.value, list(st)

    # inflate alone, alternated
    hs, ds = [], []
    for _ in range(a.repeat):
        s, rc, n, par = host_inflate(path)
        assert rc == 0 and n == len(text) and par == 1, (rc, n, par)
        hs.append(s)
        s, rc, n, st = dev_inflate(path)
        assert rc == 0 and n == len(text), (rc, n)
        ds.append(s)
    res["inflate_host_s"] = [round(x, 3) for x in hs]
    res["inflate_device_s"] = [round(x, 3) for x in ds]
    res["inflate_host_gbps"] = round(len(text) / min(hs) / 1e9, 2)
    res["inflate_device_gbps"] = round(len(text) / min(ds) / 1e9, 2)
    res["device_stats"] = dict(zip(("decoders", "accepted", "device_bytes", "host_bytes", "slabs", "members"), st))
    # text digest (untimed): the device's text against the synthesized text
    out = os.path.join(d, "dev.txt")
    dev_inflate(path, out)
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for blk in iter(lambda: f.read(1 << 26), b""):
            h.update(blk)
    res["text_digest_equal"] = h.hexdigest() == hashlib.sha256(text).hexdigest()
    os.remove(out)
    if not a.no_table:
        os.environ["JASPER_INGEST_GZ_THREADS"] = str(a.threads)
        t = KmerTable(a.k, min_slots=1 << 28)

        def to_table(p, mode):
            os.environ["JASPER_INGEST_GZ"] = mode
            t.clear()
            s = time.perf_counter()
            t.count_files([p])
            t.sync()
            s = time.perf_counter() - s
            return s, t.histogram(), t.last_inflate()
        tab = {"host": [], "device": []}
        histos = {}
        for _ in range(a.repeat):
            for mode in ("host", "device"):
                s, hg, st = to_table(path, mode)
                tab[mode].append(round(s, 3))
                histos[mode] = hg
                res["table_stats_" + mode] = st
        res["table_host_s"], res["table_device_s"] = tab["host"], tab["device"]
        res["histogram_equal"] = histos["host"] == histos["device"]
        # size sweep (file -> table, best of the repeats): where the device starts to win
        sweep = []
        for mb in [int(x) for x in a.sweep_mb.split(",") if x]:
            npc = max(1, (mb << 20) // PIECE) if mb >= 8 else 1
            sp = os.path.join(d, "sweep.fastq.gz")
            tl = write_member(sp, pieces, text, npc) if mb >= 8 else None
            if mb < 8:        # (below one piece: a gzip of a prefix)
                import gzip
                tl = (mb << 20) // REC * REC
                with open(sp, "wb") as f:
                    f.write(gzip.compress(text[:tl], 6, mtime=0))
            row = {"text_mb": round(tl / 2**20, 1), "gz_mib": round(os.path.getsize(sp) / 2**20, 2)}
            for mode in ("host", "device"):
                row[mode + "_s"] = round(min(to_table(sp, mode)[0] for _ in range(a.repeat)), 4)
            sweep.append(row)
        res["sweep"] = sweep
        t.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
