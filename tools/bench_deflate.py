"""The GPU compressor (KmerTable.deflate_bgzf) on 64 MiB of FASTQ shaped as the trio workload's -- `@r`, 150 random bases, `+`, 150 x `I`
-- five timed calls after a warm-up (HIP events), the output's size and counters, and whether gzip gives the text back; one JSON line.

    python tools/bench_deflate.py [path/to/another/libjasper_hip.so]

The optional argument loads an experiment build of the library (make OUT=... OBJDIR=... EXTRA=-DJK_DF_THREADS=512), which is how the
workgroup sizes of DESIGN.md 4.15.3 were compared (profiles/round27/variants.jsonl).
"""
import gzip
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jasper_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
from jasper_amd import KmerTable  # noqa: E402


def main():
    rng = np.random.default_rng(1)
    n, rl = 64 << 20, 150
    nreads = n // (2 * rl + 7) + 1
    rec = np.empty((nreads, 3 + rl + 3 + rl + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + rl] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (nreads, rl))]
    rec[:, 3 + rl:6 + rl] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + rl:6 + 2 * rl] = ord("I")
    rec[:, -1] = 10
    text = rec.reshape(-1)[:n].copy()
    t = KmerTable(21, min_slots=1 << 12)
    got = [t.deflate_bgzf(text) for _ in range(6)]
    secs = sorted(g[2] for g in got[1:])
    print(json.dumps({"lib": sys.argv[1:] or "default", "text_bytes": n, "median_seconds": secs[2], "seconds": secs, "bytes": int(len(got[-1][0])), "counters": got[-1][1],
                      "round_trip": gzip.decompress(got[-1][0].tobytes()) == text.tobytes()}))
    t.close()


if __name__ == "__main__":
    main()
