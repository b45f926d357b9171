"""CPU: the het-cluster half of the indel scan.  The restatement of its semantics that the GPU tests compare against
(test_gpu_het_clusters.py, test_gpu_cli_het_clusters.py), checked here against a plain form by enumeration, on planted haplotype pairs
and on the committed dumps of the golden cases; and the host side (jasper_amd/hetclusters.py: the TSV, VCF and log texts; the flag
errors of the driver and of kmerqc) on hand-made records.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h, jasper_indel_scan_clusters): s of n bytes, case folded; cnt = the count of a canonical k-mer, clamped to
2^32-1; FRONT = 64; thre >= 1, k >= 2, 1 <= N = cluster_len <= 64.
  candidate (p, x)   the window s[p-k+1 .. p] is k bases, x != s[p], cnt(F + x) >= thre with F = s[p-k+1 .. p-1]
  repl(p, R, y)      1 <= R <= N, y of t bases, 1 <= t <= N, y[0] = x: A = F + y + G_R, G_R = s[p+R .. p+R+k-2]; evaluated when all bytes
                     s[p-k+1 .. p+R+k-2] exist and are bases; ref_min(R) = the minimum over the k+R-1 windows of s that start at
                     p-k+1 .. p+R-1.  R_max = the largest R <= N that is evaluated with ref_min(R) >= thre, or 0: then the candidate is
                     not searched.  Normal form: y[t-1] != s[p+R-1] and (R, t) != (1, 1).
  search             S_1 = {x}.  After level t's record test a prefix y is closed -- not extended -- when the last k-1 bases of F + y are
                     s[p+R-k+1 .. p+R-1] for some R in 1..R_max.  S_(t+1) = the one-base extensions yz of the prefixes of S_t that are not
                     closed, with cnt(the last k bases of F + yz) >= thre.  It ends at the first of: t > N, S_t empty, |S_t| > FRONT -- then
                     the candidate is complex, counted once; the records of lengths < t stay and nothing of length >= t is listed.
  records            every (R, y), y in a reached level, 1 <= R <= R_max, in normal form, whose windows t .. t+k-2 of A are >= thre:
                     (seq, pos = p, ref_len = R, len = t, y, ref_min(R), alt_min = the minimum over all k-1+t windows of A)
  ordered by (seq, pos, ref_len, len, y); per sequence (searched, sites, records, complex), sites = searched candidates with a record."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import Case, case_names
from test_gpu_copies import as_bytes, dict_counter, kmer_dict
from test_indels_host import ACGT, U32, rand_bases
from test_indels_host import restate as restate_indels
from test_indels_mixed_host import plant_strings

FRONT = 64


def _finish(recs, per_seq):
    recs.sort(key=lambda r: (r[0], r[1], r[2], r[3], r[4]))
    counts = []
    for si, (searched, complex_) in enumerate(per_seq):
        mine = [r for r in recs if r[0] == si]
        counts.append((searched, len({(r[1], r[4][0]) for r in mine}), len(mine), complex_))
    return counts, recs


def restate_clusters(seqs, k, count, thre, N, stats=None):
    """(counts, records) of the semantics above; count(bytes of k upper-case bases) -> int.  Shortcuts: R_max from one pass over the
    reference windows, the frontier carried from level to level with its running minimum, the rejoin windows left at the first one
    below thre.  stats, a dict, gets `candidates`, `searched`, `complex`, `widest` (the largest level that was searched) and `levels`
    (the sizes of all levels t >= 2 that were computed, those above FRONT too)."""
    recs, per_seq = [], []
    st = dict(candidates=0, searched=0, complex=0, widest=0, levels=[])
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        n = len(up)
        isb = [ch in ACGT for ch in up]
        searched = complex_ = 0
        run = 0                                                   # bases in a row that end at p
        for p in range(n):
            run = run + 1 if isb[p] else 0
            if run < k:
                continue
            F = up[p - k + 1:p]
            cands = [x for x in ACGT if x != up[p] and min(count(F + bytes([x])), U32) >= thre]
            if not cands:
                continue
            st["candidates"] += len(cands)
            # R_max and ref_min(1 .. R_max)
            rmins, m, j = [], U32, p - k + 1
            for R in range(1, N + 1):
                if p + R + k - 2 > n - 1 or not isb[p + R + k - 2] or (R == 1 and not all(isb[p + 1:p + k - 1])):
                    break
                while j <= p + R - 1:
                    m = min(m, min(count(up[j:j + k]), U32))
                    j += 1
                if m < thre:
                    break
                rmins.append(m)
            Rmax = len(rmins)
            if Rmax == 0:
                continue
            closers = {up[p + R - k + 1:p + R] for R in range(1, Rmax + 1)}
            for x in cands:
                searched += 1
                xb = bytes([x])
                S, t = [(xb, min(count(F + xb), U32))], 1
                while True:
                    st["widest"] = max(st["widest"], len(S))
                    for y, m0 in S:
                        for R in range(1, Rmax + 1):
                            if y[-1] == up[p + R - 1] or (R == 1 and t == 1):
                                continue
                            alt = (F + y + up[p + R:p + R + k - 1])[t:]      # windows t .. t+k-2
                            amin = m0
                            for w in range(k - 1):
                                amin = min(amin, min(count(alt[w:w + k]), U32))
                                if amin < thre:
                                    break
                            if amin >= thre:
                                recs.append((si, p, R, t, y.decode(), rmins[R - 1], amin))
                    if t == N:
                        break
                    new = []
                    for y, m0 in S:
                        if (F + y)[-(k - 1):] in closers:
                            continue
                        for z in ACGT:
                            c = min(count((F + y + bytes([z]))[-k:]), U32)
                            if c >= thre:
                                new.append((y + bytes([z]), min(m0, c)))
                    st["levels"].append(len(new))
                    if len(new) > FRONT:
                        complex_ += 1
                        break
                    if not new:
                        break
                    S, t = new, t + 1
        per_seq.append((searched, complex_))
        st["searched"] += searched
        st["complex"] += complex_
    if stats is not None:
        stats.update(st)
    return _finish(recs, per_seq)


def restate_clusters_plain(seqs, k, count, thre, N):
    """the same straight from the definition: every p, x and R, every string y of every length, every minimum over all its windows; a
    level S_t as the set of strings of length t that start with x, whose t windows of F + y are solid and none of whose shorter
    prefixes is closed"""
    recs, per_seq = [], []
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        n = len(up)
        searched = complex_ = 0

        def cmin(a):
            return min(min(count(a[j:j + k]), U32) for j in range(len(a) - k + 1))

        def bases(lo, hi):
            return 0 <= lo and hi <= n - 1 and all(ch in ACGT for ch in up[lo:hi + 1])

        for p in range(n):
            if not bases(p - k + 1, p):
                continue
            F = up[p - k + 1:p]
            Rmax = 0
            for R in range(1, N + 1):
                if bases(p - k + 1, p + R + k - 2) and cmin(up[p - k + 1:p + R + k - 1]) >= thre:
                    Rmax = R
            for x in ACGT:
                xb = bytes([x])
                if x == up[p] or min(count(F + xb), U32) < thre or Rmax == 0:
                    continue
                searched += 1

                def closed(y):
                    return any((F + y)[-(k - 1):] == up[p + R - k + 1:p + R] for R in range(1, Rmax + 1))

                levels = {}
                for t in range(1, N + 1):
                    level = []
                    for rest in itertools.product(ACGT, repeat=t - 1):
                        y = xb + bytes(rest)
                        if cmin(F + y) >= thre and not any(closed(y[:u]) for u in range(1, t)):
                            level.append(y)
                    if not level:
                        break
                    if len(level) > FRONT:
                        complex_ += 1
                        break
                    levels[t] = level
                for t, level in levels.items():
                    for y in level:
                        for R in range(1, Rmax + 1):
                            if y[-1] == up[p + R - 1] or (R, t) == (1, 1):
                                continue
                            amin = cmin(F + y + up[p + R:p + R + k - 1])
                            if amin >= thre:
                                recs.append((si, p, R, t, y.decode(), cmin(up[p - k + 1:p + R + k - 1]), amin))
        per_seq.append((searched, complex_))
    return _finish(recs, per_seq)


def substitute(s, at):
    """s with the bytes at the given positions replaced by the next base (A -> C -> G -> T -> A)"""
    b = bytearray(s)
    for p in at:
        b[p] = ACGT[(ACGT.index(b[p]) + 1) & 3]
    return bytes(b)


def applied(contig, rec):
    """the contig with one record put in place of what it replaces"""
    _, pos, rlen, _, y, _, _ = rec
    return contig[:pos] + y.encode() + contig[pos + rlen:]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def tiny_fuzz(k, seed=517):
    """reads that hold two haplotypes twice each: pairs of substitutions close together, a substitution beside a length difference;
    contigs: either haplotype, one with an N and lower case, short ones"""
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, 110)
    h = plant_strings(substitute(g, [20, 22, 50, 51, 80]), [(83, "del", 1)])
    a = bytearray(g)
    a[65] = ord("N")
    a[15:30] = bytes(a[15:30]).lower()
    return [g] * 2 + [h] * 2, [g, h, bytes(a), g[:k], b"", g[40:40 + 2 * k + 2]]


def test_the_restatement_agrees_with_its_plain_form():
    seen = dict(records=0, complex=0, searched=0)
    for k in (3, 4, 5):
        reads, seqs = tiny_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        for thre, N in ((1, 1), (1, 4), (2, 3), (2, 5), (3, 4)):
            got = restate_clusters(seqs, k, count, thre, N)
            assert got == restate_clusters_plain(seqs, k, count, thre, N), (k, thre, N)
            for c in got[0]:
                seen["searched"] += c[0]
                seen["records"] += c[2]
                seen["complex"] += c[3]
            assert all(c[1] <= c[0] and c[1] <= c[2] for c in got[0])
    assert seen["records"] > 20 and seen["searched"] > 20, seen


def planted_pairs(k, seed=188):
    """(h1, h2, [(p, d)], far): two haplotypes that differ by pairs of substitutions at p and p + d for d in 1, 2, 3, 7, k-2, k-1, one
    pair every 4k bases, and by one pair k apart (far = its first position)"""
    rng = np.random.default_rng(seed + k)
    ds = (1, 2, 3, 7, k - 2, k - 1)
    h1 = rand_bases(rng, 4 * k * (len(ds) + 2))
    at, pairs = [], []
    for i, d in enumerate(ds):
        p = 2 * k + 4 * k * i
        at += [p, p + d]
        pairs.append((p, d))
    far = 2 * k + 4 * k * len(ds)
    return h1, substitute(h1, at + [far, far + k]), pairs, far


@pytest.mark.parametrize("k", [21, 31, 64])
def test_planted_pairs(k):
    """two SNPs d < k apart, five copies of each haplotype: exactly one record (p, d+1, d+1, the other haplotype's bytes) from either
    side, and applying it gives the other haplotype there; k apart they are two isolated sites of the variant scan and list nothing"""
    h1, h2, pairs, far = planted_pairs(k)
    count = dict_counter(kmer_dict([h1] * 5 + [h2] * 5, k))
    for mine, other in ((h1, h2), (h2, h1)):
        st = {}
        counts, recs = restate_clusters([mine], k, count, 3, 64, st)
        assert recs == [(0, p, d + 1, d + 1, other[p:p + d + 1].decode(), 5, 5) for p, d in pairs]
        assert counts == [(len(pairs) + 2, len(pairs), len(pairs), 0)] and st["widest"] == 1      # (the far pair: two searched candidates)
        for r in recs:
            got = applied(mine, r)
            assert got[r[1] - k:r[1] + r[2] + k] == other[r[1] - k:r[1] + r[2] + k] and got != mine
        # N = d + 1 lists the pair, N = d does not
        for p, d in pairs[:4]:
            assert [r[1] for r in restate_clusters([mine], k, count, 3, d + 1)[1]] == [q for q, e in pairs if e <= d]
            assert [r[1] for r in restate_clusters([mine], k, count, 3, d)[1]] == [q for q, e in pairs if e < d]


def snp_beside_indel(k, seed=266):
    """(longer, shorter, p): two haplotypes that differ by a substitution at p and, 6 bases on, by 2 bytes that only the longer holds;
    the bytes around the length difference are chosen so that it has one position only"""
    rng = np.random.default_rng(seed + k)
    while True:
        g = rand_bases(rng, 8 * k)
        p = 3 * k
        q = p + 6
        if g[q + 1] != g[q - 1] and g[q] != g[q + 2] and g[q + 1] != g[q + 3] and g[q - 1] != g[q + 1] and g[q - 2] != g[q] and g[q + 2] != g[q + 1]:
            return g, plant_strings(substitute(g, [p]), [(q, "del", 2)]), p


@pytest.mark.parametrize("k", [21, 31, 64])
def test_a_snp_beside_a_length_difference(k):
    longer, shorter, p = snp_beside_indel(k)
    count = dict_counter(kmer_dict([longer] * 5 + [shorter] * 5, k))
    a = restate_clusters([longer], k, count, 3, 64)
    b = restate_clusters([shorter], k, count, 3, 64)
    assert a[0] == [(1, 1, 1, 0)] and b[0] == [(1, 1, 1, 0)]
    ra, rb = a[1][0], b[1][0]
    assert ra[1] == p and rb[1] == p and ra[2] - ra[3] == 2 and rb[3] - rb[2] == 2 and ra[5:] == (5, 5) and rb[5:] == (5, 5)
    assert (ra[2], ra[3]) in ((8, 6), (9, 7)) and (rb[2], rb[3]) in ((6, 8), (7, 9))      # (right-normalisation may shift it by a base)
    assert applied(longer, ra) == shorter[:p] + shorter[p:] and applied(shorter, rb) == longer


def test_the_closure_rule():
    """a pair k apart, and two isolated het sites 40 apart at k = 21 with N = 64: each is the variant scan's, and no union is listed"""
    k = 21
    rng = np.random.default_rng(2121)
    h1 = rand_bases(rng, 400)
    for at in ([150, 150 + k], [150, 190], [150, 190, 230]):
        h2 = substitute(h1, at)
        count = dict_counter(kmer_dict([h1] * 5 + [h2] * 5, k))
        for mine in (h1, h2):
            st = {}
            counts, recs = restate_clusters([mine], k, count, 3, 64, st)
            assert recs == [] and counts == [(len(at), 0, 0, 0)] and st["widest"] == 1
            assert st["levels"].count(1) == len(at) * (k - 1) and st["levels"].count(0) == len(at) and len(st["levels"]) == len(at) * k      # closed after k - 1 bases back on the contig


def test_pure_insertions_and_deletions_are_the_indel_scan_s():
    """normal form: a difference of length alone is never listed here, and the indel restatement lists it"""
    k = 21
    rng = np.random.default_rng(909)
    h1 = rand_bases(rng, 600)
    h2 = plant_strings(h1, [(150, "ins", b"G" if h1[150] != ord("G") else b"C"), (300, "del", 3), (450, "ins", b"GAT" if h1[450] != ord("G") else b"CAT")])
    count = dict_counter(kmer_dict([h1] * 5 + [h2] * 5, k))
    for mine in (h1, h2):
        counts, recs = restate_clusters([mine], k, count, 3, 64)
        assert recs == [] and counts[0][0] >= 3 and counts[0][1:] == (0, 0, 0)
        assert len(restate_indels([mine], k, count, 3, 4)[1]) >= 2


def cap_workload():
    """(reads, contigs) at k = 4 and thre 1: one read of 90 random bases and a contig cut from it; in so small a k-mer space the levels
    of a candidate grow past FRONT within a few bases"""
    rng = np.random.default_rng(285)
    g = rand_bases(rng, 90)
    return [g], [g[20:60]]


def test_a_level_wider_than_the_front_is_complex_once():
    reads, seqs = cap_workload()
    count = dict_counter(kmer_dict(reads, 4))
    st5, st6 = {}, {}
    want5, want6 = restate_clusters(seqs, 4, count, 1, 5, st5), restate_clusters(seqs, 4, count, 1, 6, st6)
    assert want5[0][0][3] == 0 and st5["complex"] == 0 and max(st5["levels"]) <= FRONT
    assert 0 < want6[0][0][3] == st6["complex"] == sum(1 for n in st6["levels"] if n > FRONT) <= want6[0][0][0] == want5[0][0][0]
    assert st6["widest"] <= FRONT < max(st6["levels"]) and len(want6[1]) > len(want5[1])      # complex once each, and the shorter records stay
    assert want5 == restate_clusters_plain(seqs, 4, count, 1, 5) and want6 == restate_clusters_plain(seqs, 4, count, 1, 6)


def dense_workload():
    """k = 5, 280 random bases read once and scanned at thre 1 with N = 64: far more records than candidates"""
    rng = np.random.default_rng(55)
    g = rand_bases(rng, 280)
    return [g], [g]


# ---- anchors on the committed dumps ----------------------------------------------------------------------------------------------
SEARCHED = {"diploid_k25": 10, "rolling_k25": 17, "rolling_k37": 17}      # searched candidates at N = 64; 0 in every other case
WIDEST = {"rolling_k25": 7, "rolling_k37": 9}                            # the widest level; 1 where anything is searched


@pytest.mark.parametrize("name", case_names())
def test_golden_anchors(name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    st = {}
    counts, recs = restate_clusters(seqs, c.k, count, c.thre, 64, st)
    assert recs == [] and st["complex"] == 0, (name, recs)
    assert st["searched"] == SEARCHED.get(name, 0) == sum(x[0] for x in counts), (name, st["searched"])
    assert st["widest"] == (WIDEST.get(name, 1) if st["searched"] else 0), (name, st["widest"])


def test_the_anchors_name_golden_cases():
    assert set(SEARCHED) | set(WIDEST) <= set(case_names()) and len(case_names()) == 17


# ---- writers ---------------------------------------------------------------------------------------------------------------------
def test_tsv_and_log_texts():
    from jasper_amd import hetclusters
    names = ["c1", "c2"]
    stages = [("before", [100, 50], [(4, 3, 5, 1), (1, 0, 0, 2)]), ("after", [99, 50], [(1, 1, 1, 0), None])]      # c2: not in the polished FASTA
    assert hetclusters.het_clusters_tsv_text(names, stages) == (
        "#contig\tstage\tlength\tsearched\tsites\trecords\tcomplex\n"
        "c1\tbefore\t100\t4\t3\t5\t1\nc1\tafter\t99\t1\t1\t1\t0\n"
        "c2\tbefore\t50\t1\t0\t0\t2\nc2\tafter\t0\t0\t0\t0\t0\n"
        "*\tbefore\t150\t5\t3\t5\t3\n*\tafter\t99\t1\t1\t1\t0\n")
    assert hetclusters.het_clusters_tsv_text(["c"], [("asm", [7], [(0, 0, 0, 0)])]) == (
        "#contig\tstage\tlength\tsearched\tsites\trecords\tcomplex\nc\tasm\t7\t0\t0\t0\t0\n*\tasm\t7\t0\t0\t0\t0\n")
    assert hetclusters.stage_log_text(stages[0][2]) == "5 searched, 3 sites, 5 records, 3 complex"
    assert hetclusters.log_text(stages[0][2], stages[1][2]) == ("Het clusters: before polishing 5 searched, 3 sites, 5 records, 3 complex; "
                                                                "after polishing 1 searched, 1 sites, 1 records, 0 complex")


def test_vcf_text():
    from jasper_amd import hetclusters
    from jasper_amd.table import HET_CLUSTER_DTYPE, HetClusters
    long_y = "ACGT" * 16
    names, seqs = ["c1", "c2"], ["GATTacaTCAGAGAGCTN", "ACGTACGTAC" * 8]
    recs = [(1, 3, 64, 64, long_y[1:] + "A", 11, 4),           # c2: len 64, as long as what it replaces
            (0, 4, 3, 3, "GCT", 8, 7),                         # c1: POS 5, REF aca as it stands in the file, an MNP
            (0, 4, 3, 2, "GT", 8, 9),                          # c1: the same site, shorter than REF: complex, before the MNP (LEN)
            (0, 4, 3, 3, "CCT", 8, 6),                         # c1: the same site and length: ALT order
            (0, 4, 2, 5, "TTGCA", 9, 3),                       # c1: the same site, a shorter REF: first (RLEN)
            (0, 9, 2, 5, "TTGCA", 5, 3)]                       # c1: longer than REF: complex
    txt = hetclusters.vcf_text(31, 3, 64, names, [18, 80], seqs, recs)
    head = [ln for ln in txt.splitlines() if ln.startswith("#")]
    body = [ln for ln in txt.splitlines() if not ln.startswith("#")]
    assert head[:4] == ["##fileformat=VCFv4.2", "##source=jasper_amd het-cluster scan, k=31, threshold=3, max_len=64", "##contig=<ID=c1,length=18>",
                        "##contig=<ID=c2,length=80>"]
    assert [ln.split(",")[0] for ln in head[4:-1]] == ["##INFO=<ID=%s" % x for x in ("KIND", "TYPE", "RLEN", "LEN", "RC", "AC")]
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert body == ["c1\t5\t.\tac\tTTGCA\t.\t.\tKIND=het;TYPE=complex;RLEN=2;LEN=5;RC=9;AC=3",
                    "c1\t5\t.\taca\tGT\t.\t.\tKIND=het;TYPE=complex;RLEN=3;LEN=2;RC=8;AC=9",
                    "c1\t5\t.\taca\tCCT\t.\t.\tKIND=het;TYPE=mnp;RLEN=3;LEN=3;RC=8;AC=6",
                    "c1\t5\t.\taca\tGCT\t.\t.\tKIND=het;TYPE=mnp;RLEN=3;LEN=3;RC=8;AC=7",
                    "c1\t10\t.\tAG\tTTGCA\t.\t.\tKIND=het;TYPE=complex;RLEN=2;LEN=5;RC=5;AC=3",
                    "c2\t4\t.\t%s\t%s\t.\t.\tKIND=het;TYPE=mnp;RLEN=64;LEN=64;RC=11;AC=4" % (seqs[1][3:67], long_y[1:] + "A")]
    # the same from a structured array in another order and from sequences as bytes; record_tuples gives the tuples back
    arr = np.zeros(len(recs), dtype=HET_CLUSTER_DTYPE)
    for i, (seq, pos, rlen, ln, y, rmin, amin) in enumerate(reversed(recs)):
        v = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(y))
        arr[i] = (pos, seq, rmin, amin, rlen, [v & (2**64 - 1), v >> 64], ln, [0] * 6)
    assert hetclusters.vcf_text(31, 3, 64, names, [18, 80], [s.encode() for s in seqs], arr) == txt
    hc = HetClusters([], arr, 0.0, 0, False)
    assert hc.record_tuples() == list(reversed(recs))
    assert [ln for ln in hetclusters.vcf_text(31, 3, 64, names, [18, 80], seqs, []).splitlines() if not ln.startswith("#")] == []


def test_files_are_written_through_a_tmp_name(tmp_path):
    from jasper_amd import hetclusters
    fn = str(tmp_path / "x.het_clusters.tsv")
    hetclusters.write_atomic(fn, "abc\n")
    assert open(fn).read() == "abc\n" and os.listdir(str(tmp_path)) == ["x.het_clusters.tsv"]


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def _run(module, args, cwd):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)


def _inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "r.fa"
    fq.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    return ["-a", str(fa), "-r", str(fq), "-k", "5"]


@pytest.mark.parametrize("module", ["jasper_amd.cli", "jasper_amd.kmerqc"])
@pytest.mark.parametrize("bad", ["0", "65", "-1", "x", "6.5"])
def test_a_bad_length_ends_the_run(module, bad, tmp_path):
    args = _inputs(tmp_path) + ["--indels", "--het-clusters", "--het-cluster-max-len", bad] + (["--threshold", "1"] if module.endswith("kmerqc") else [])
    r = _run(module, args, tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--het-cluster-max-len takes an integer from 1 to 64; it is %s" % bad in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


@pytest.mark.parametrize("module", ["jasper_amd.cli", "jasper_amd.kmerqc"])
def test_het_clusters_needs_indels(module, tmp_path):
    args = _inputs(tmp_path) + ["--het-clusters"] + (["--threshold", "1"] if module.endswith("kmerqc") else [])
    r = _run(module, args, tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--het-clusters needs --indels" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


def test_the_flag_functions():
    from jasper_amd import cli
    assert cli.het_cluster_flags(None) == 64 and cli.het_cluster_flags("1") == 1 and cli.het_cluster_flags("64") == 64
