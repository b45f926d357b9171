"""GPU: runs placed by window index, one layout for the three run scans (k-mer report, copy-number scan, hap-mer scan without a child).

The three kernels find their runs the same way: a 16-bit class mask per thread of a tile of TILE windows, a run start where a class bit
follows a window without it (the thread before's bit 15 carried over), a walk through the masks that takes whole groups of 16 at once, and
partial runs stitched across tile seams.  The layout below puts a run at every position where that can go wrong; RANGES says which.

Every canonical k-mer of the three sequences occurs once (asserted on the CPU before anything runs on the GPU), so a window's count is how
often the substring of its range -- windows [a, b) are the bases seq[a : b - 1 + K] -- was put into the counted text, N-separated.  What is
expected is computed here from RANGES alone, never from the library, and compared exactly, through the host-text and the device-text entry
point; no scan may need its repeat."""
import functools
from collections import Counter

import pytest

from test_gpu_copies import TILE
from test_gpu_scan_stage import on_device, rand_bases

pytestmark = pytest.mark.gpu

K, SEED = 21, 17
WINDOWS = (TILE + 64, TILE + 64, 2 * TILE + 2200)
# (sequence, first window, end, kind): half open; the kinds are those of the two-class scans (1 = excess / mat, 2 = deficit / pat), the report
# has one class and makes one run of two ranges that touch
RANGES = (
    (0, 0, 1, 1),                              # the tile's first window
    (0, 15, 17, 2),                            # across two threads' groups: carried over by the thread before's bit 15
    (0, 32, 48, 1),                            # exactly one aligned group: the whole-group path
    (0, 63, 97, 2),                            # part of a group, two whole groups, one window
    (0, TILE - 3, TILE + 2, 1),                # across the seam
    (1, TILE - 16, TILE, 1),                   # up to the seam, and from the seam on the other kind: two runs, in the report one of 21
    (1, TILE, TILE + 5, 2),
    (2, 100, 100 + TILE + 2000, 1),            # one run through two seams
)
ONCE = (0, 80, 97)                             # the report's counted text holds these windows (the second half of (0, 63, 97)) once: below thre 2, not absent

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def pieces(si):
    """sequence si cut into (first window, end, kind) in order, kind 0 = the background between the ranges"""
    out, cur = [], 0
    for s, a, b, kind in RANGES:
        if s != si:
            continue
        assert cur <= a < b <= WINDOWS[si]
        if a > cur:
            out.append((cur, a, 0))
        out.append((a, b, kind))
        cur = b
    if cur < WINDOWS[si]:
        out.append((cur, WINDOWS[si], 0))
    return out


def text(seqs, times, extra=()):
    """the counted text: every piece's substring times[kind] times, and those of `extra` (sequence, first window, end) once"""
    parts = []
    for si, s in enumerate(seqs):
        for a, b, kind in pieces(si):
            parts += [s[a:b - 1 + K]] * times[kind]
    parts += [seqs[si][a:b - 1 + K] for si, a, b in extra]
    return b"N".join(parts)


@functools.lru_cache(maxsize=None)
def layout():
    import numpy as np
    rng = np.random.default_rng(SEED)
    seqs = [rand_bases(rng, nw + K - 1) for nw in WINDOWS]
    canon = Counter()
    for s in seqs:
        for i in range(len(s) - K + 1):
            km = s[i:i + K]
            canon[min(km, km.translate(_COMP)[::-1])] += 1
    assert len(canon) == sum(WINDOWS) and max(canon.values()) == 1      # every window has a k-mer of its own
    return seqs


def two_class_runs():
    return [(s, a, b - a, kind) for s, a, b, kind in RANGES]


def class_windows(si, kind):
    return sum(b - a for a, b, kd in pieces(si) if kd == kind)


class Scans:
    def __init__(self, KT, seqs):
        def table(t):
            T = KT(K, min_slots=1 << 17)
            T.count_bases(t)
            return T
        self.seqs = seqs
        self.report = table(text(seqs, {0: 2, 1: 0, 2: 0}, [ONCE]))
        self.reads = table(text(seqs, {0: 4, 1: 8, 2: 1}))
        self.asm = table(b"N".join(seqs))
        self.mat = table(text(seqs, {0: 1, 1: 1, 2: 0}))
        self.pat = table(text(seqs, {0: 1, 1: 0, 2: 1}))
        self.d_text, self.offs = on_device(seqs)

    def close(self):
        for t in (self.report, self.reads, self.asm, self.mat, self.pat):
            t.close()


@pytest.fixture(scope="module")
def scans(request):
    seqs = layout()                            # (its assertion comes before the library is loaded)
    request.getfixturevalue("hip")
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    s = Scans(KmerTable, seqs)
    yield s
    s.close()


def both_entries(host, device):
    for what, res in (("host text", host()), ("device text", device())):
        assert not res.retried, what
        yield what, res


def test_report_runs(scans):
    want_runs = []
    for s, a, b, _ in RANGES:                  # one class: ranges that touch are one run
        if want_runs and want_runs[-1][0] == s and want_runs[-1][1] + want_runs[-1][2] == a:
            a = want_runs.pop()[1]
        want_runs.append((s, a, b - a))
    once = lambda s, a, b: max(0, min(b, ONCE[2]) - max(a, ONCE[1])) if s == ONCE[0] else 0      # noqa: E731
    want_runs = [(s, a, n, n - once(s, a, a + n), 0 if n > once(s, a, a + n) else 1) for s, a, n in want_runs]
    assert (0, 63, 34, 17, 0) in want_runs and (1, TILE - 16, 21, 21, 0) in want_runs and len(want_runs) == 7
    want_counts = []
    for si, nw in enumerate(WINDOWS):
        unrel = nw - class_windows(si, 0)
        want_counts.append((nw, nw, unrel, unrel - once(si, 0, nw)))
    T = scans.report
    for what, rep in both_entries(lambda: T.kmer_report(scans.seqs, 2), lambda: T.kmer_report_device(scans.d_text, scans.offs, 2)):
        assert rep.counts == want_counts, what
        assert rep.run_tuples() == want_runs, what


def test_copy_runs(scans):
    want_runs = [(s, a, n, kind, (8 if kind == 1 else 1) * n, n) for s, a, n, kind in two_class_runs()]
    want_counts = []
    for si, nw in enumerate(WINDOWS):
        bg, ex, de = (class_windows(si, kind) for kind in (0, 1, 2))
        want_counts.append((nw, nw, ex, de, 4 * bg + 8 * ex + de, nw))
    R, A = scans.reads, scans.asm
    for what, rep in both_entries(lambda: R.copy_report(A, scans.seqs, 1, 4), lambda: R.copy_report_device(A, scans.d_text, scans.offs, 1, 4)):
        assert rep.counts == want_counts, what
        assert rep.run_tuples() == want_runs, what


def test_hapmer_runs(scans):
    from jasper_amd import KmerTable
    want_runs = two_class_runs()
    want_counts = [(nw, nw, class_windows(si, 1), class_windows(si, 2)) for si, nw in enumerate(WINDOWS)]
    M, P = scans.mat, scans.pat
    for what, rep in both_entries(lambda: KmerTable.hapmer_scan_parents(M, P, scans.seqs, 1, 1),
                                  lambda: M.hapmer_scan_device(M, P, scans.d_text, scans.offs, 1, 1, child=False)):
        assert rep.counts == want_counts, what
        assert rep.run_tuples() == want_runs, what
