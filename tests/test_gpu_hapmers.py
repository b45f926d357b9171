"""GPU: the trio hap-mer scan (KmerTable.hapmer_scan / hapmer_scan_device / hapmer_scan_parents, jasper_hapmer_scan) against a
restatement of its semantics fed by Python dicts of canonical k-mer strings.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): window i of a sequence of n bytes exists for 0 <= i <= n-k and is valid iff all k bytes are
ACGTacgt; m, p, c = its canonical k-mer's counts in the mother's table M, the father's P and the child's R, clamped to 2^32-1; class
mat (1) iff valid, m >= thre_mat, p == 0 and (no child table or c >= thre_child); class pat (2) iff valid, p >= thre_pat, m == 0 and
the same; else 0.  Per sequence (windows, valid, mat, pat); a run is a maximal range of consecutive windows of one sequence with the
same non-zero class: (seq, start, n_kmers, kind), ordered by (seq, start)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
TILE = 4096
MAT, PAT = 1, 2
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def kmer_dict(seqs, k, times=1):
    """canonical k-mer (bytes) -> occurrences over the sequences, each taken `times` times: upper-cased, every maximal stretch of
    >= k ACGT bytes walked"""
    d = {}
    for s in seqs:
        for m in re.finditer(rb"[ACGT]{%d,}" % k, as_bytes(s).upper()):
            t = m.group()
            for i in range(len(t) - k + 1):
                km = t[i:i + k]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                d[key] = d.get(key, 0) + times
    return d


def window_keys(seq, k):
    """per window: None (not valid) or its canonical k-mer"""
    b = as_bytes(seq)
    n = len(b)
    pre = [0] * (n + 1)
    for i, ch in enumerate(b):
        pre[i + 1] = pre[i] + (0 if ch in b"ACGTacgt" else 1)
    up = b.upper()
    out = []
    for i in range(max(0, n - k + 1)):
        if pre[i + k] != pre[i]:
            out.append(None)
            continue
        km = up[i:i + k]
        rc = km.translate(_COMP)[::-1]
        out.append(km if km < rc else rc)
    return out


def restate(seqs, k, md, pd, cd, tm, tp, tc):
    """(counts, runs) of the semantics above; cd None = no child table"""
    counts, runs = [], []
    for si, s in enumerate(seqs):
        keys = window_keys(s, k)
        valid = nm = np_ = 0
        cur = None
        for i, key in enumerate(keys):
            cls = 0
            if key is not None:
                valid += 1
                m, p = min(md.get(key, 0), U32), min(pd.get(key, 0), U32)
                kept = cd is None or min(cd.get(key, 0), U32) >= tc
                if m >= tm and p == 0 and kept:
                    cls = MAT
                elif p >= tp and m == 0 and kept:
                    cls = PAT
                nm += cls == MAT
                np_ += cls == PAT
            if cur is not None and cur[3] != cls:
                runs.append(tuple(cur))
                cur = None
            if cls:
                if cur is None:
                    cur = [si, i, 0, cls]
                cur[2] += 1
        if cur is not None:
            runs.append(tuple(cur))
        counts.append((len(keys), valid, nm, np_))
    return counts, runs


def check(rep, want, what):
    want_counts, want_runs = want
    assert rep.counts == want_counts, what
    got = rep.run_tuples()
    assert len(got) == len(want_runs), (what, len(got), len(want_runs))
    assert got == want_runs, what


def tile_ends_crossed(r):
    """tile ends strictly inside the run: windows i, i+1 both in the run with i+1 a multiple of TILE"""
    return (r[1] + r[2] - 1) // TILE - r[1] // TILE


def rand_seq(rng, n):
    return bytearray(BASES[rng.integers(0, 4, n)].tobytes())


def snp(seq, pos, rng=None):
    """another base at pos (the next one in ACGT order, or a random other one)"""
    i = b"ACGT".index(seq[pos])
    seq[pos] = b"ACGT"[(i + (1 if rng is None else int(rng.integers(1, 4)))) % 4]


def depth(text, d):
    """a parent "at depth d": its haplotype text d times, joined by a separator byte"""
    return b"N".join([bytes(text)] * d)


def table(KT, k, text, min_slots=1 << 16):
    t = KT(k, min_slots=min_slots)
    t.count_bases(bytes(text))
    return t


def is_wide(t):
    """the low 64 remainder bits of a slot's key are in a second array when 2k - log2(slots) > 53 (csrc/kmer.hpp: wide_rem)"""
    return 2 * t.k - (t.info()["slots"].bit_length() - 1) > 53


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


DEPTH, THRE = 3, 2


def make_trio(seed, k, windows, seam_snps=()):
    """a random base sequence of `windows` windows; the maternal and the paternal haplotype differ from it by independent SNPs about
    every 400 bases (the maternal one also at seam_snps); the child contig is the maternal haplotype up to the middle, the paternal one
    after it.  -> (mat hap, pat hap, contig)"""
    rng = np.random.default_rng(seed)
    n = windows + k - 1
    base = rand_seq(rng, n)
    haps = []
    for extra in (seam_snps, ()):
        h = bytearray(base)
        for pos in sorted(set(rng.choice(n, max(1, n // 400), replace=False).tolist()) | set(extra)):
            snp(h, pos, rng)
        haps.append(h)
    mid = n // 2
    return bytes(haps[0]), bytes(haps[1]), bytes(haps[0][:mid] + haps[1][mid:])


class Trio:
    """the three tables of make_trio and the dicts they were made from: parents at depth DEPTH, the child both haplotypes at depth 2"""

    def __init__(self, KT, seed, k, windows, seam_snps=()):
        self.k = k
        self.mat_hap, self.pat_hap, self.contig = make_trio(seed, k, windows, seam_snps)
        self.md, self.pd = kmer_dict([self.mat_hap], k, DEPTH), kmer_dict([self.pat_hap], k, DEPTH)
        self.cd = kmer_dict([self.mat_hap, self.pat_hap], k, 2)
        self.M, self.P = table(KT, k, depth(self.mat_hap, DEPTH)), table(KT, k, depth(self.pat_hap, DEPTH))
        self.R = table(KT, k, depth(self.mat_hap, 2) + b"N" + depth(self.pat_hap, 2))

    def want(self, seqs, child=True, tm=THRE, tp=THRE, tc=THRE):
        return restate(seqs, self.k, self.md, self.pd, self.cd if child else None, tm, tp, tc)

    def close(self):
        for t in (self.M, self.P, self.R):
            t.close()


@pytest.fixture(scope="module")
def trio25(KT):
    k = 25
    t = Trio(KT, 2501, k, 3 * TILE + 100, seam_snps=(TILE + 5, 2 * TILE + 3))      # their k windows straddle a tile seam
    yield t
    t.close()


def trio_seqs(t):
    """the contig, an empty sequence, k - 1 and exactly k bytes, a piece with separators and lower case inside markers, and a second contig"""
    k, c = t.k, t.contig
    piece = bytearray(c[TILE - 300:TILE + 900])
    marked = [r for r in t.want([bytes(piece)])[1]]
    assert len(marked) >= 2
    a, b = marked[0], marked[1]             # a separator in the middle of one marker, lower case over another
    piece[a[1] + a[2] // 2 + k // 2] = ord("N")
    lo, hi = b[1], b[1] + b[2] + k - 1
    piece[lo:hi] = bytes(piece[lo:hi]).lower()
    return [c, b"", c[:k - 1], c[100:100 + k], bytes(piece), t.pat_hap[:5000]]


def test_trio_across_tiles(KT, trio25):
    t = trio25
    seqs = trio_seqs(t)
    want = t.want(seqs)
    rep = t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE)
    print(want[0], len(want[1]), rep.seconds)
    check(rep, want, "trio k=25")
    kinds = [r[3] for r in want[1] if r[0] == 0]
    assert kinds.count(MAT) >= 10 and kinds.count(PAT) >= 10, "vacuous case"
    assert sum(tile_ends_crossed(r) for r in want[1]) >= 2, "no run crosses a tile seam"
    assert want[0][1] == (0, 0, 0, 0) and want[0][2] == (0, 0, 0, 0) and want[0][3][0] == 1
    assert any(r[0] == 4 for r in want[1]) and want[0][4][1] < want[0][4][0]
    assert rep.seconds > 0 and not rep.retried
    # without the child: at least the same markers
    rep0 = t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE, child=False)
    check(rep0, t.want(seqs, child=False), "trio k=25, no child")
    assert KT.hapmer_scan_parents(t.M, t.P, seqs, THRE, THRE) == rep0


@pytest.mark.parametrize("kind", [MAT, PAT])
def test_a_run_longer_than_a_tile(KT, kind):
    """a 9 000-base insertion only one parent holds: one run that covers a whole middle tile (the stitch's chain through a tile whose
    only partial run spans it)"""
    k = 25
    rng = np.random.default_rng(90 + kind)
    left, ins, right = bytes(rand_seq(rng, 2000)), bytes(rand_seq(rng, 9000)), bytes(rand_seq(rng, 2000))
    contig = left + ins + right
    has, lacks = depth(contig, DEPTH), depth(left + b"N" + right, DEPTH)
    hd, ld = kmer_dict([contig], k, DEPTH), kmer_dict([left, right], k, DEPTH)
    md, pd = (hd, ld) if kind == MAT else (ld, hd)
    M, P = table(KT, k, has if kind == MAT else lacks), table(KT, k, lacks if kind == MAT else has)
    R = table(KT, k, depth(contig, 2))
    want = restate([contig], k, md, pd, kmer_dict([contig], k, 2), THRE, THRE, THRE)
    assert want[1] == [(0, 2000 - k + 1, 9000 + k - 1, kind)] and tile_ends_crossed(want[1][0]) == 2
    check(R.hapmer_scan(M, P, [contig], THRE, THRE, THRE), want, "long run")
    check(KT.hapmer_scan_parents(M, P, [contig, contig[100:]], THRE, THRE), restate([contig, contig[100:]], k, md, pd, None, THRE, THRE, 1), "long run, two contigs")
    for t in (M, P, R):
        t.close()


def test_touching_runs_of_different_kinds(KT):
    """a maternal-only allele at x and a paternal-only one at x + k: windows x-k+1 .. x are mat, x+1 .. x+k pat -- two runs that touch,
    with x the last window of a tile"""
    k = 25
    rng = np.random.default_rng(33)
    x = TILE - 1
    base = rand_seq(rng, 2 * TILE + k - 1)
    contig, mh, ph = bytearray(base), bytearray(base), bytearray(base)
    snp(contig, x)
    snp(mh, x)
    snp(contig, x + k)
    snp(ph, x + k)
    contig = bytes(contig)
    md, pd = kmer_dict([mh], k, DEPTH), kmer_dict([ph], k, DEPTH)
    M, P = table(KT, k, depth(mh, DEPTH)), table(KT, k, depth(ph, DEPTH))
    want = restate([contig], k, md, pd, None, THRE, THRE, 1)
    assert want[1] == [(0, x - k + 1, k, MAT), (0, x + 1, k, PAT)] and (x + 1) % TILE == 0
    check(KT.hapmer_scan_parents(M, P, [contig], THRE, THRE), want, "touching runs")
    # the same pair away from the seam, and the kinds the other way round
    want = restate([contig[7:]], k, pd, md, None, THRE, THRE, 1)
    assert want[1] == [(0, x - 7 - k + 1, k, PAT), (0, x - 7 + 1, k, MAT)]
    check(KT.hapmer_scan_parents(P, M, [contig[7:]], THRE, THRE), want, "touching runs, swapped")
    M.close()
    P.close()


def plant(kmers_and_counts):
    """single k-mers as separator-joined strings, each `count` times"""
    return b"N".join(b"N".join([km] * c) for km, c in kmers_and_counts if c > 0) + b"N"


def test_threshold_edges(KT):
    k, tm, tp, tc = 21, 4, 3, 5
    rng = np.random.default_rng(44)
    contig = bytes(rand_seq(rng, 400))
    w = lambda i: contig[i:i + k]
    assert len(kmer_dict([contig], k)) == len(contig) - k + 1
    m_plan = [(w(10), tm - 1), (w(12), tm)] + [(w(i), tm) for i in range(50, 60)] + [(w(i), 1) for i in range(100, 104)] + [(w(201), 1)]
    p_plan = [(w(55), 1)] + [(w(i), tp) for i in range(100, 104)] + [(w(200), tp - 1), (w(201), tp), (w(202), tp)] + [(w(300), 1)]
    c_plan = [(w(i), tc) for i in (10, 12, 50, 51, 53, 54, 55, 56, 57, 58, 59, 200, 201, 202)] + [(w(52), tc - 1), (w(300), tc + 7)]
    mt, pt, ct = plant(m_plan), plant(p_plan), plant(c_plan)
    md, pd, cd = kmer_dict([mt], k), kmer_dict([pt], k), kmer_dict([ct], k)
    M, P, R = table(KT, k, mt), table(KT, k, pt), table(KT, k, ct)
    want = restate([contig], k, md, pd, cd, tm, tp, tc)
    # 10: one below the threshold; 12: at it; 50..59 split by p == 1 at 55 and by the child's count at 52; 100..103 in both parents;
    # 200: below the father's threshold, 201: the mother has it once, 202: pat; 300: the father's threshold is above its count
    assert want[1] == [(0, 12, 1, MAT), (0, 50, 2, MAT), (0, 53, 2, MAT), (0, 56, 4, MAT), (0, 202, 1, PAT)]
    check(R.hapmer_scan(M, P, [contig], tm, tp, tc), want, "threshold edges")
    want = restate([contig], k, md, pd, None, tm, tp, tc)
    assert want[1] == [(0, 12, 1, MAT), (0, 50, 5, MAT), (0, 56, 4, MAT), (0, 202, 1, PAT)]
    check(R.hapmer_scan(M, P, [contig], tm, tp, tc, child=False), want, "threshold edges, child=False")
    check(KT.hapmer_scan_parents(M, P, [contig], tm, tp), want, "threshold edges, no child table")
    # thresholds of 1: everything a parent holds alone
    check(R.hapmer_scan(M, P, [contig], 1, 1, 1), restate([contig], k, md, pd, cd, 1, 1, 1), "thresholds of 1")
    for t in (M, P, R):
        t.close()


@pytest.mark.parametrize("k", [19, 41, 63])
def test_other_k(KT, k):
    t = Trio(KT, 1900 + k, k, TILE - 7)
    seqs = [t.contig, t.contig[:k - 1], t.contig[k:3 * k].lower() + b"N" + t.contig[500:900]]
    want = t.want(seqs)
    assert sum(r[3] == MAT for r in want[1]) >= 3 and sum(r[3] == PAT for r in want[1]) >= 3
    if k == 63:
        assert is_wide(t.M) and is_wide(t.P) and is_wide(t.R)
    check(t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE), want, "k=%d" % k)
    check(t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE, child=False), t.want(seqs, child=False), "k=%d, no child" % k)
    t.close()


def test_more_runs_than_the_first_buffer_holds(KT):
    """the mother holds the k-mers at the even windows of a random sequence only: 80 000 runs of one window each are more than the
    scan's first list of partial runs has room for (windows / 64 + 65 536)"""
    k, windows = 21, 160_000
    rng = np.random.default_rng(77)
    s = bytes(rand_seq(rng, windows + k - 1))
    assert len(kmer_dict([s], k)) == windows, "a k-mer occurs twice: the count below would not be what this test claims"
    mt = b"N".join(s[i:i + k] for i in range(0, windows, 2))
    pt = b"A" * k
    md, pd = kmer_dict([mt], k), kmer_dict([pt], k)
    assert not set(pd) & set(kmer_dict([s], k))
    want = restate([s], k, md, pd, None, 1, 1, 1)
    assert len(want[1]) == windows // 2 > windows // 64 + 65_536 and all(r[2] == 1 and r[3] == MAT for r in want[1])
    M, P = table(KT, k, mt), table(KT, k, pt)
    rep = KT.hapmer_scan_parents(M, P, [s], 1, 1)
    check(rep, want, "alternating")
    assert rep.retried
    M.close()
    P.close()


def histo(t):
    return list(t.histogram())


def test_entry_points_and_state(KT, trio25):
    import torch
    t = trio25
    seqs = [as_bytes(s) for s in trio_seqs(t)]
    before = histo(t.M), histo(t.P), histo(t.R)
    first = t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE)
    check(first, t.want(seqs), "host entry")
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.R.hapmer_scan_device(t.M, t.P, d, offs, THRE, THRE, THRE) == first
    assert t.R.hapmer_scan_device(t.M, t.P, d, offs, THRE, THRE, THRE, child=False) == t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE, child=False)
    assert t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE) == first
    # a copy scan and a hap-mer scan of one child table keep their own buffers
    A = table(KT, t.k, b"N".join(seqs))
    crep = t.R.copy_report(A, seqs, 1, 4)
    assert len(crep.runs) > 0
    assert t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE) == first
    assert t.R.copy_report(A, seqs, 1, 4) == crep
    assert t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE) == first
    A.close()
    assert (histo(t.M), histo(t.P), histo(t.R)) == before


def test_attached_child(KT, trio25):
    """the child's table as an attached owner-sharded one: the same result through every owner's shard; an attached parent is refused"""
    from test_gpu_shard import make_shards
    t = trio25
    seqs = trio_seqs(t)
    slots = t.R.info()["slots"]
    shards, _ = make_shards(KT, t.R, 2, slots)
    for o, s in enumerate(shards):
        s.attach_tables(shards, o)
    want = t.want(seqs)
    check(shards[0].hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE), want, "attached child, owner 0")
    check(shards[1].hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE), want, "attached child, owner 1")
    with pytest.raises(Exception, match="maternal table must be a whole table"):
        t.R.hapmer_scan(shards[0], t.P, seqs, THRE, THRE, THRE)
    with pytest.raises(Exception, match="paternal table must be a whole table"):
        t.R.hapmer_scan(t.M, shards[1], seqs, THRE, THRE, THRE)
    for s in shards:
        s.close()


def test_error_cases(KT, hip, trio25):
    """every cause of include/jasper_hip.h but one by its message.  "different devices" needs a second GPU: on a machine with one -- the
    usual test machine -- that case cannot be made and does not run; the others do not depend on it.  An attached M or P is in
    test_attached_child, an attached A in test_gpu_hapmer_census.py."""
    import ctypes as C
    from jasper_amd import _lib
    t = trio25
    seqs = [t.contig[:500]]
    other = table(KT, 27, t.contig[:2000])
    with pytest.raises(Exception, match="different k"):
        t.R.hapmer_scan(t.M, other, seqs, THRE, THRE, THRE)
    with pytest.raises(Exception, match="different k"):
        other.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE)
    other.close()
    with pytest.raises(Exception, match="maternal table and the paternal table are the same table"):
        t.R.hapmer_scan(t.M, t.M, seqs, THRE, THRE, THRE)
    with pytest.raises(Exception, match="maternal table and the child table are the same table"):
        t.M.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE)
    with pytest.raises(Exception, match="paternal table and the child table are the same table"):
        t.P.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE)
    for bad, who in (((0, THRE, THRE), "maternal"), ((THRE, 0, THRE), "paternal"), ((THRE, THRE, 0), "child")):
        with pytest.raises(Exception, match="%s threshold must be at least 1" % who):
            t.R.hapmer_scan(t.M, t.P, seqs, *bad)
    n = C.c_int(0)
    _lib.check(hip.jasper_device_count(C.byref(n)))
    if n.value >= 2:                         # (a second GPU is not always there: the other causes do not need one)
        far = KT(t.k, min_slots=1 << 16, device=1)
        far.count_bases(t.contig[:2000])
        with pytest.raises(Exception, match="different devices"):
            t.R.hapmer_scan(t.M, far, seqs, THRE, THRE, THRE)
        far.close()
    # and nothing above has changed what a good call returns
    check(t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE), t.want(seqs), "after the refusals")
