"""Planted polishing workloads whose position classes are known by construction, and a restatement of the polisher's cut rule
(jasper_amd/csrc/polish.hip: find_sync_batch_kernel, find_clean_batch_kernel; polish_plan.hpp: plan_cuts, which
tests/test_polish_plan_host.py holds against this restatement).  No GPU use.

The workload.  A random truth without a repeated canonical k-mer; error-free reads: pieces of the truth, C times each, 'N'
between them.  A window that a piece covers has count C (solid), any other count 0, and no window is OTHER (no count is 50
times another).  Chunks are slices of the truth, so coordinates below are TRUTH coordinates unless they say otherwise:

  sub at e        the chunk text differs from the truth at e: exactly the windows e-k+1 .. e are BAD, and a fixing pass that
                  restores the truth leaves them CLEAN
  dip (d, r)      no read piece covers the windows d .. d+r-1 (pieces end at d+k-1 and start again at d+r): a BAD run of chosen
                  length in a correct text, which no pass changes

The sequential walk (src/jasper.py:55-100) steps k-1 windows at a time from the chunk's window 0 until it stands on a BAD window;
a one-window dip is counted (one bad k-mer) iff the walk stands exactly on it, and the walk goes on from the window after it: every
counted dip moves the stride phase by one.  walk_hits() restates that for texts of CLEAN and BAD windows.
"""
import numpy as np

CLEAN, BAD = 0, 1
C_READS, THRE = 2, 2          # every covered window is seen twice; a window is solid from 2


def geometry(k):
    """{TMIN, CMIN, CLEAN_CELL, W, M}: the library's own numbers (a query, no GPU call)"""
    from jasper_amd import KmerTable
    return KmerTable.polish_cut_geometry(k)


_TRUTHS = {}


def truth(k, n, seed):
    """random ACGT text of n bases in which no canonical k-mer occurs twice (checked with the oracle's map)"""
    key = (k, n, seed)
    if key not in _TRUTHS:
        from oracle import oracle as O
        t = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()
        db = O.OracleDB(k)
        db.count_bases(t)
        assert db.distinct() == n - k + 1, "the truth repeats a canonical k-mer: take another seed"
        _TRUTHS[key] = t.decode()
    return _TRUTHS[key]


class Plant:
    """one truth, its dips, and chunks (lo, hi, subs) cut from it"""

    def __init__(self, k, truth_text, dips=(), chunks=(), passes=0, name=""):
        self.k, self.truth, self.passes, self.name = k, truth_text, passes, name
        self.dips = sorted((int(d), int(r)) for d, r in dips)
        self.chunks = [(int(lo), int(hi), sorted(int(e) for e in subs)) for lo, hi, subs in chunks]
        at = 0
        self.pieces = []
        for d, r in self.dips:
            assert r >= 1 and d + k - 1 - at >= k, "dips too close for a read piece between them"
            self.pieces.append((at, d + k - 1))
            at = d + r
        assert len(truth_text) - at >= k
        self.pieces.append((at, len(truth_text)))
        for lo, hi, subs in self.chunks:
            assert 0 <= lo <= hi <= len(truth_text) and all(lo <= e < hi for e in subs)

    def reads(self):
        """bytes: every piece C_READS times, 'N' between"""
        return "N".join(self.truth[a:b] for a, b in self.pieces for _ in range(C_READS)).encode()

    def names(self):
        return ["%s%d:%d" % (self.name or "c", i, lo) for i, (lo, _, _) in enumerate(self.chunks)]

    def seqs(self, prepend=0):
        """chunk texts; `prepend`: that many more truth bases in front of every chunk (another stride phase for everything in it)"""
        out = []
        for lo, hi, subs in self.chunks:
            assert lo >= prepend
            t = list(self.truth[lo - prepend:hi])
            for e in subs:
                t[e - lo + prepend] = "ACGT"[("ACGT".index(t[e - lo + prepend]) + 1) % 4]
            out.append("".join(t))
        return out

    def classes(self, ci, pass_i):
        """class of every window of chunk ci at the start of pass pass_i (pass 0: dips and subs; later: dips only -- the tests
        establish with the oracle that pass 0 restores the truth)"""
        lo, hi, subs = self.chunks[ci]
        k = self.k
        nwin = max(0, hi - lo - k + 1)
        cls = np.zeros(nwin, dtype=np.uint8)
        for d, r in self.dips:
            a, b = max(0, d - lo), min(nwin, d + r - lo)
            if a < b:
                cls[a:b] = BAD
        if pass_i == 0:
            for e in subs:
                a, b = max(0, e - lo - k + 1), min(nwin, e - lo + 1)
                if a < b:
                    cls[a:b] = BAD
        return cls

    def segments(self, geo=None):
        """segments the polisher's accounting reports for the whole call: the first cut of every chunk in every pass, QV pass included"""
        geo = geo or geometry(self.k)
        total = 0
        for ci, (lo, hi, _) in enumerate(self.chunks):
            for p in range(self.passes + 1):
                total += len(cuts(self.classes(ci, min(p, 1)), hi - lo, self.k, geo)) + 1
        return total


# ---- the cut rule -------------------------------------------------------------------------------------------------------

def sync_candidates(cls, k, W):
    """find_sync_batch_kernel: p is BAD after CLEAN, p .. p+k-2 all BAD, the W windows before p all CLEAN, p >= W, p+k-1 <= nwin"""
    nwin = len(cls)
    out = []
    starts = np.nonzero((cls[1:] == BAD) & (cls[:-1] == CLEAN))[0] + 1 if nwin > 1 else []
    for p in (int(x) for x in starts):
        if p < W or p + k - 1 > nwin:
            continue
        if (cls[p:p + k - 1] == BAD).all() and (cls[p - W:p] == CLEAN).all():
            out.append(p)
    return out


def clean_cells(cls, k, cell):
    """find_clean_batch_kernel: per cell of `cell` windows, starting at its middle, a p whose windows [p-4k, p+k) are all CLEAN,
    or -1; a failed attempt moves p to 4k+1 behind the last window in the way; at most 8 attempts, inside the text and the cell"""
    nwin = len(cls)
    out = []
    for g in range(nwin // cell + 1):
        p0, cand = g * cell + cell // 2, -1
        for _ in range(8):
            if p0 - 4 * k < 0 or p0 + k > nwin or p0 + k > (g + 1) * cell:
                break
            bad = np.nonzero(cls[p0 - 4 * k:p0 + k] != CLEAN)[0]
            if not len(bad):
                cand = p0
                break
            p0 = p0 - 4 * k + int(bad[-1]) + 4 * k + 1
        out.append(cand)
    return out


def cuts(cls, length, k, geo):
    """plan_cuts: [(position, chained)] of one chunk of `length` bases in one pass; its segments are one more"""
    TMIN, CMIN = geo["TMIN"], geo["CMIN"]
    nwin = length - k + 1
    assert len(cls) == max(0, nwin)
    sync, last = [], 0
    if nwin > 2 * TMIN:                                     # want_sync
        for p in sorted(sync_candidates(cls, k, geo["W"])):
            if p - last >= TMIN and length - p >= TMIN:
                sync.append(p)
                last = p
    out = [(p, 0) for p in sync]
    if nwin > 2 * CMIN:
        out, si, last = [], 0, 0
        for p in clean_cells(cls, k, geo["CLEAN_CELL"]) + [None]:
            while si < len(sync) and (p is None or sync[si] <= p):
                out.append((sync[si], 0))
                last = sync[si]
                si += 1
            if p is None or p < 0:
                continue
            nxt = sync[si] if si < len(sync) else length
            if p - last >= CMIN and nxt - p >= CMIN:
                out.append((p, 1))
                last = p
    return out


# ---- the walk over CLEAN / BAD windows ----------------------------------------------------------------------------------------

def walk_hits(cls, k):
    """first window of every BAD run the sequential walk stands on (the walk goes on from the first good window behind the run)"""
    nwin, i, hits = len(cls), 0, []
    bad = np.nonzero(cls != CLEAN)[0]
    while i < nwin:
        if cls[i] != CLEAN:
            hits.append(i)
            while i < nwin and cls[i] != CLEAN:
                i += 1
            continue
        j = int(np.searchsorted(bad, i))
        if j == len(bad):
            break
        steps = max(1, (int(bad[j]) - i) // (k - 1))      # (straight to the last stop before the next BAD window)
        i += steps * (k - 1)
    return hits


def steer(k, lo, base, target):
    """one-window dips (truth coordinates, from `base` on, 4 strides apart) that the walk of a chunk starting at `lo` stands on
    one after the other, after which it stands on truth window `target`: each one moves the phase by one"""
    s = k - 1
    n = (target - lo) % s
    first = lo + ((base - lo + s - 1) // s) * s
    dips = [(first + 4 * s * j + j, 1) for j in range(n)]
    assert not dips or dips[-1][0] + 8 * k < target
    return dips


# ---- the plants the tests use (tests/test_polish_cuts_host.py fixes their expectations, tests/test_gpu_polish_paths.py runs them) ----

LO = 128                      # every chunk starts this far into its truth: room to prepend k-2 bases for the other stride phases
KS = (21, 37, 63)             # (63: the widest k the oracle holds)


CUT_NAMES = ("spacing_-1", "spacing_+0", "spacing_+1", "first_-1", "first_+0", "last_-1", "last_+0", "nwin_2T", "nwin_2T+1",
             "left_neighbour_legal", "left_neighbour_too_close", "nwin_2C", "nwin_2C+1", "clean_cuts_3", "second_attempt_ref",
             "second_attempt", "dip_left_of_cut", "dip_right_of_cut", "attempts_8_fail", "attempts_7_fail")      # cut_plants(k)
PHASE_NAMES = ("behind_one_clean", "behind_one_clean_off_stride", "behind_dirty_then_clean")                     # phase_plants(k)


def _sub_at(p, k):
    """truth position of the substitution whose BAD run starts at chunk window p"""
    return LO + p + k - 1


def cut_plants(k):
    """{name: Plant} -- sync points around TMIN and the nearest legal left neighbour (substitutions, one fixing pass), clean
    cuts around CMIN and around dips (QV pass only).  One chunk each."""
    g = geometry(k)
    T, CM, CELL, W = g["TMIN"], g["CMIN"], g["CLEAN_CELL"], g["W"]
    small = truth(k, 8192, 100 + k)
    big = truth(k, 300_000 + LO, 200 + k)
    out = {}

    def subs_plant(name, length, cands, tr=small):
        out[name] = Plant(k, tr, (), [(LO, LO + length, [_sub_at(p, k) for p in cands])], passes=1, name=name)

    def dips_plant(name, length, dips_chunk, tr=big):
        out[name] = Plant(k, tr, [(LO + d, r) for d, r in dips_chunk], [(LO, LO + length, [])], passes=0, name=name)

    for s in (T - 1, T, T + 1):
        subs_plant("spacing_%+d" % (s - T), 6000, [2000, 2000 + s])
    for p in (T - 1, T):
        subs_plant("first_%+d" % (p - T), 4000, [p])
        subs_plant("last_%+d" % (p - T), 4000, [4000 - p])
    subs_plant("nwin_2T", 2 * T + k - 1, [T])
    subs_plant("nwin_2T+1", 2 * T + k, [T])
    p = T + 80                                     # its left neighbour's own run starts before TMIN: not a sync point itself
    subs_plant("left_neighbour_legal", 4000, [p - W - k, p])          # that run ends at p - W - 1
    subs_plant("left_neighbour_too_close", 4000, [p - W - k + 1, p])  # ... at p - W: p is no candidate
    dips_plant("nwin_2C", 2 * CM + k - 1, [])
    dips_plant("nwin_2C+1", 2 * CM + k, [])
    dips_plant("clean_cuts_3", 300_000, [])
    p0 = CELL + CELL // 2                          # the second cell's middle; the chunk ends CMIN behind it
    st = lambda target: [(d - LO, r) for d, r in steer(k, LO, LO + 2000, LO + target)]
    dips_plant("second_attempt_ref", p0 + CM, [])
    dips_plant("second_attempt", p0 + CM, st(p0 - 4 * k) + [(p0 - 4 * k, 1)])
    p = CELL // 2                                  # the cut taken in the first cell
    dips_plant("dip_left_of_cut", 2 * CELL, st(p - 4 * k - 1) + [(p - 4 * k - 1, 1)])
    dips_plant("dip_right_of_cut", 2 * CELL, st(p + k) + [(p + k, 1)])
    dips_plant("attempts_8_fail", 100_000, [(p + k - 1 + 5 * k * j, 1) for j in range(8)])
    dips_plant("attempts_7_fail", 100_000, [(p + k - 1 + 5 * k * j, 1) for j in range(7)])
    return out


def _on_stride(x, k):
    return (x + k - 2) // (k - 1) * (k - 1)


def phase_plants(k, long_chain=False):
    """{name: (Plant, on_stride)} -- a one-window dip that the walk counts only if the arrival handed down a chain of segments has
    the right phase (on_stride False: the dip lies one window off, and must not be counted).  QV pass only, one chunk each."""
    g = geometry(k)
    CM, CELL = g["CMIN"], g["CLEAN_CELL"]
    big = truth(k, 300_000 + LO, 200 + k)
    out = {}

    def plant(name, tr, length, dips_chunk, on):
        out[name] = (Plant(k, tr, [(LO + d, r) for d, r in dips_chunk], [(LO, LO + length, [])], passes=0, name=name), on)

    x = _on_stride(CELL + CELL // 2 + 6000, k)                 # in the third segment: behind the first one and a clean chained one
    plant("behind_one_clean", big, 300_000, [(x, 1)], True)
    plant("behind_one_clean_off_stride", big, 300_000, [(x + 1, 1)], False)
    y = _on_stride(CELL // 2 + 6000, k)                        # counted in the second segment: the phase moves by one there
    x = _on_stride(3 * CELL + CELL // 2 + 6000, k) + 1         # in the fifth segment, on the moved stride
    plant("behind_dirty_then_clean", big, 300_000, [(y, 1), (x, 1)], True)
    if long_chain:
        n = 72                                                 # cuts; 71 clean chained segments between the first and the last
        tr = truth(k, n * CELL + CM + LO, 300 + k)
        x = _on_stride((n - 1) * CELL + CELL // 2 + 6000, k)
        plant("behind_71_clean", tr, n * CELL + CM, [(x, 1)], True)
    return out


def ragged_batch(k):
    """(Plant, extra texts): long chunks with substitutions, a chunk of k+3, an empty one, chunks on both sides of 2*TMIN + k - 1,
    and -- as extra texts, outside the plant's bookkeeping -- a slice of the truth with random substitutions, insertions and
    deletions, some of them closer than k (fix records of every kind, the ones with aux bytes included)"""
    from jasper_amd import synth
    T = geometry(k)["TMIN"]
    tr = truth(k, 520_000, 400 + k)
    rng = np.random.default_rng(k)

    def subs(lo, hi, every):
        return [int(e) for e in range(lo + 700, hi - 700, every)]
    chunks = [(LO, LO + 150_000, subs(LO, LO + 150_000, 1531)),
              (160_000, 160_000 + k + 3, []),
              (161_000, 161_000, []),
              (162_000, 162_000 + 2 * T + k - 1, [162_000 + T + k - 1]),
              (166_000, 166_000 + 2 * T + k, [166_000 + T + k - 1]),
              (170_000, 310_000, subs(170_000, 310_000, 40_009)),
              (320_000, 380_000, subs(320_000, 380_000, 2903))]
    messy = synth.make_assembly(rng, np.frombuffer(tr[400_000:500_000].encode(), dtype=np.uint8), err=3e-3, n_every=10**9).tobytes().decode()
    return Plant(k, tr, (), chunks, passes=2, name="r"), [("messy:400000", messy)]
