#!/usr/bin/env python3
"""The counting path's integers, call by call, for comparing two builds of the library (GPU box):

    JASPER_AMD_LIB=other/libjasper_hip.so python tools/count_crosscheck.py > other.jsonl
    python tools/count_crosscheck.py > this.jsonl          # the two files must be equal

One JSON line per counting call: what JASPER_COUNT_DEBUG=2 says of its pieces -- the geometry of every partitioned piece, the
`piece done` sequence (position, distinct keys, table size, dup_ratio; the millisecond fields are left out), the two recovery paths
where they are taken -- then count_stages()'s path and partitioned-launch count, info(), a checksum of the histogram, and
exchange_plan's eight words for 2, 4 and 8 owners at three piece sizes.  Inputs: bench.py's, the texts of
tests/test_gpu_count_text.py at k = 16, 37, 38 and 64, a call whose size hint is too small (the restart with worst-case sizing) and
the planted input of tests/test_gpu_parity.py whose partitioned piece abandons itself."""
import hashlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stream_ref as sr  # noqa: E402
from jasper_amd import KmerTable, synth  # noqa: E402

DEV = torch.device("cuda", 0)
GEOM = re.compile(r"\[count\] (partitioned piece \d+ bases: p1 \d+ p2 \d+ rbits \d+ nblk1 \d+ nblk2 \d+ cap1 \d+ cap2 \d+) \|")
DONE = re.compile(r"\[count\] (piece done: pos \d+ / \d+, distinct \d+, slots 2\^\d+, dup_ratio [0-9.]+),")
PATHS = re.compile(r"\[count\] (partitioned piece abandoned|size hint too small for this input)")
PLAN_PIECES = (3_000_000, 47_000_000, 1 << 30)


def counted(t, ptr, n):
    """one counting call with the library's stderr caught -> the lines that say what the host decided, in order"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["JASPER_COUNT_DEBUG"] = "2"
        try:
            t.count_bases_device(ptr, n)
        finally:
            del os.environ["JASPER_COUNT_DEBUG"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        log = f.read().decode()
    out = []
    for ln in log.split("\n"):
        for pat in (GEOM, DONE, PATHS):
            m = pat.search(ln)
            if m:
                out.append(m.group(1))
    return out


def line(call, t, pieces):
    _, parts = t.count_stages()
    plans = {}
    for nown in (2, 4, 8):
        for piece in PLAN_PIECES:
            p = t.exchange_plan(piece, nown)
            plans["%d/%d" % (nown, piece)] = None if p is None else [int(v) for v in p.values()]      # (the eight words; p2 as its two halves)
    histo = hashlib.sha256(np.array(t.histogram(), dtype=np.uint64).tobytes()).hexdigest()[:16]
    print(json.dumps(dict(call=call, pieces=pieces, path=int(t.count_path()), partitioned=int(parts), info={k: int(v) for k, v in t.info().items()}, histo=histo, plans=plans)),
          flush=True)


def count_text(name, k, text, shift=0, slots=1 << 24, calls=1):
    buf = torch.full((text.size + 32,), ord("A"), dtype=torch.uint8, device=DEV)
    view = buf[shift:shift + text.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(text)).to(DEV))
    torch.cuda.synchronize()
    t = KmerTable(k, min_slots=slots)
    for c in range(calls):
        line("%s/k%d/call%d" % (name, k, c), t, counted(t, view.data_ptr(), text.size))
    t.close()
    del buf, view
    torch.cuda.empty_cache()


def main():
    # bench.py's input
    import bench as B
    torch.cuda.set_device(0)
    reads, _, _, _, _, _, nreads = B.build_workload(torch, DEV, 0, 1, 47.0, 2)
    t = KmerTable(B.K, min_slots=max(1 << 21, int(1.25 * int(nreads * 150 * 2.1 / 10))))
    for c in range(2):                            # (the second call: into the filled table)
        line("bench/call%d" % c, t, counted(t, reads.data_ptr(), reads.numel()))
    t.close()
    del reads
    torch.cuda.empty_cache()
    # the texts of tests/test_gpu_count_text.py
    TILE, PERIOD, S = 16384, 2_000_003, 24
    LEN = 8 * 2**20 + 3 * TILE + 5
    ROOM = 3 * (1 << S) // 4
    LEN_LONG = ROOM + 8 * 2**20 + 2 * TILE + 7
    base = sr.base_text(LEN_LONG, PERIOD)
    for k in (16, 37, 38, 64):
        count_text("base", k, base[:LEN], calls=2)
        count_text("seam", k, sr.seam_text(base[:LEN], k, TILE)[0])
        count_text("runs", k, sr.run_text(base[:LEN], TILE, 76, 175)[0])
    for shift in (0, 9):
        count_text("long/shift%d" % shift, 37, sr.seam_text(base, 37, TILE)[0], shift=shift)
    # a size hint that is too small: 20 M bases without a repeat into a table asked for 2^20 keys
    gen = torch.Generator(device=DEV).manual_seed(77)
    genome = synth.torch_genome(gen, 20_000_000, DEV)
    torch.cuda.synchronize()
    t = KmerTable(31, min_slots=1 << 20)
    line("hint_too_small", t, counted(t, genome.data_ptr(), genome.numel()))
    t.close()
    del genome
    # tests/test_gpu_parity.py, test_one_kmer_that_makes_up_much_of_the_input[0.10-37]: the partitioned piece abandons itself
    gen = torch.Generator(device=DEV).manual_seed(5)
    genome = synth.torch_genome(gen, 1_500_000, DEV)
    nreads = 1_500_000 * 30 // 150
    reads = synth.torch_reads_stream(gen, genome, nreads, 150, 0.004)
    m = int(reads.numel() * 0.10) // 151 * 151
    reads[:m].view(-1, 151)[:, :150] = ord("A")
    torch.cuda.synchronize()
    t = KmerTable(37, min_slots=int(1.25 * nreads * 150 * 2.1 / 10))
    for c in range(2):
        line("abandoned/call%d" % c, t, counted(t, reads.data_ptr(), reads.numel()))
    t.close()


if __name__ == "__main__":
    main()
