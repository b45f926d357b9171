"""CPU: the gap scan.  The restatement of its semantics that the GPU tests compare against (test_gpu_gaps.py, test_gpu_cli_gaps.py),
checked here against a plain form by enumeration, on planted gaps and on the site rules; the host side (jasper_amd/gaps.py: the TSV,
BED, fill and log texts and fill_sequences; the flag errors of the driver and of kmerqc) on hand-made sites and records; and
jasper_amd/csrc/gaps_host.hpp as a stand-alone program under sanitizers, on the same site cases.  Nothing expected here comes from the
code under test.

Semantics (include/jasper_hip.h, jasper_gap_scan): s case folded; cnt = the count of a canonical k-mer, clamped to 2^32-1; FRONT = 64,
MAXREC = 16; thre >= 1, k >= 2, 0 <= max_len <= 4096, max_trim >= 0.  A window is valid when its k bytes are bases, solid when valid
and cnt >= thre.
  sites    a stretch = a maximal run [u0, u1] of windows that are not solid.  kind gap: it holds an invalid window; kind run: none, and
           u1 - u0 + 2 - k > 64 (only with long_runs); else no site.  a = u0 + k - 1, q = u1 + 1, F = s[a-k+1 .. a), G = s[q .. q+k-1).
           edge: u0 = 0 or u1 = n - k (trims 0).  Else ragged: trim_left = (first non-base byte) - a or trim_right = q - (last non-base
           byte + 1) exceeds max_trim.  Else searched.  ref_min = the smallest cnt over the stretch's valid windows, 0 without one.
  search   S_0 = {empty}; at level t = 0, 1, ..: (1) rejoin: every y in S_t whose windows t .. t+k-2 of F + y + G are solid is a record;
           more than MAXREC with the site's earlier ones: none of the level is listed, complex, levels = t.  (2) close: y with t >= k - 1
           and its last k - 1 bases equal to G leaves S_t.  (3) t = max_len: limit if S_t is not empty, else dead; S_t empty: dead;
           levels = t.  (4) S_(t+1) = the one-base extensions whose newest window is solid; more than FRONT: complex; none: dead;
           levels = t + 1 in both cases.
  records  (seq, pos = a, ref_len = R, len = t, y, ref_min, alt_min = the minimum over all t + k - 1 windows), by (seq, pos, len, y)
  counts   per sequence (sites, searched, bridged, unique, records, edge, ragged, limit, complex)"""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_compound_host import substitute
from test_gpu_copies import as_bytes, dict_counter, kmer_dict
from test_gpu_kmer_report import restate as restate_runs
from test_gpu_kmer_report import window_counts
from test_indels_host import ACGT, U32, rand_bases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT, MAXREC, RUN_MIN = 64, 16, 64
SEARCHED = ("dead", "limit", "complex")


def search_site(F, G, k, count, thre, max_len, levels=None):
    """(status, levels, [(t, y, alt_min)]) of one searched site.  Shortcuts: the frontier is carried from level to level with its running
    minimum, and the rejoin windows stop at the first one below thre.  levels, a list, gets the size of every S_(t+1) that was computed."""
    S, recs, t = [(b"", U32)], [], 0
    while True:
        lvl = []
        for y, m in S:
            alt = (F + y)[-(k - 1):] + G                              # windows t .. t+k-2
            amin = m
            for j in range(k - 1):
                amin = min(amin, min(count(alt[j:j + k]), U32))
                if amin < thre:
                    break
            if amin >= thre:
                lvl.append((t, y.decode(), amin))
        if len(recs) + len(lvl) > MAXREC:
            return "complex", t, recs
        recs += lvl
        if t >= k - 1:
            S = [(y, m) for y, m in S if y[-(k - 1):] != G]
        if t == max_len:
            return ("limit" if S else "dead"), t, recs
        if not S:
            return "dead", t, recs
        new = []
        for y, m in S:
            tail = (F + y)[-(k - 1):]
            for z in ACGT:
                c = min(count(tail + bytes([z])), U32)
                if c >= thre:
                    new.append((y + bytes([z]), min(m, c)))
        if levels is not None:
            levels.append(len(new))
        if len(new) > FRONT:
            return "complex", t + 1, recs
        if not new:
            return "dead", t + 1, recs
        S, t = new, t + 1


def search_site_plain(F, G, k, count, thre, max_len):
    """the same straight from the definition, for small max_len: every string of every length, every minimum over all its windows"""
    def cmin(x):
        return min(min(count(x[j:j + k]), U32) for j in range(len(x) - k + 1)) if len(x) >= k else U32

    def closed(y):
        return len(y) >= k - 1 and y[-(k - 1):] == G

    def member(y):              # y is in S_t as level t meets it: every window of F + y is solid and no shorter prefix was closed
        return cmin(F + y) >= thre and not any(closed(y[:i]) for i in range(len(y)))

    recs = []
    for t in range(max_len + 1):
        St = [bytes(y) for y in itertools.product(ACGT, repeat=t) if member(bytes(y))]
        lvl = [(t, y.decode(), cmin(F + y + G)) for y in St if cmin(F + y + G) >= thre]
        if len(recs) + len(lvl) > MAXREC:
            return "complex", t, recs
        recs += lvl
        left = [y for y in St if not closed(y)]
        if t == max_len:
            return ("limit" if left else "dead"), t, recs
        if not left:
            return "dead", t, recs
        nxt = sum(1 for y in itertools.product(ACGT, repeat=t + 1) if member(bytes(y)))
        if nxt > FRONT:
            return "complex", t + 1, recs
        if nxt == 0:
            return "dead", t + 1, recs


def find_sites(s, k, count, thre, max_trim, long_runs):
    """[(a, q, kind, status or None, trim_left, trim_right, ref_min)] of one sequence, from a loop over its windows and its bytes"""
    b = as_bytes(s)
    n = len(b)
    wc = window_counts(s, k, count)
    solid = [c is not None and c >= thre for c in wc]
    out, i = [], 0
    while i < len(solid):
        if solid[i]:
            i += 1
            continue
        j = i
        while j < len(solid) and not solid[j]:
            j += 1
        u0, u1 = i, j - 1
        i = j
        gap = any(wc[w] is None for w in range(u0, u1 + 1))
        if not gap and (not long_runs or u1 - u0 + 2 - k <= RUN_MIN):
            continue
        a, q = u0 + k - 1, u1 + 1
        valid = [wc[w] for w in range(u0, u1 + 1) if wc[w] is not None]
        rmin = min(valid) if valid else 0
        if u0 == 0 or u1 == n - k:
            out.append((a, q, "gap" if gap else "run", "edge", 0, 0, rmin))
            continue
        tl = tr = 0
        if gap:
            nb = [p for p in range(u0, u1 + k) if b[p:p + 1] not in (b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t")]
            tl, tr = nb[0] - a, q - (nb[-1] + 1)
        out.append((a, q, "gap" if gap else "run", "ragged" if max(tl, tr) > max_trim else None, tl, tr, rmin))
    return out


def _finish(n_seqs, sites, recs):
    recs.sort(key=lambda r: (r[0], r[1], r[3], r[4]))
    counts = []
    for si in range(n_seqs):
        mine = [s for s in sites if s[0] == si]
        counts.append((len(mine), sum(s[4] in SEARCHED for s in mine), sum(s[5] > 0 for s in mine), sum(s[5] == 1 and s[4] != "complex" for s in mine),
                       sum(s[5] for s in mine)) + tuple(sum(s[4] == st for s in mine) for st in ("edge", "ragged", "limit", "complex")))
    return counts, sites, recs


def restate_gaps(seqs, k, count, thre, max_len, max_trim, long_runs, stats=None, search=search_site):
    """(counts, sites, records) of the semantics above; count(bytes of k upper-case bases) -> int.  sites are in the order of
    GapScan.site_tuples(): (seq, a, q, kind, status, n_records, levels, trim_left, trim_right, ref_min).  stats, a dict, gets `levels`: the
    level sizes of every search, one list per searched site."""
    sites, recs, lv = [], [], []
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        for a, q, kind, status, tl, tr, rmin in find_sites(s, k, count, thre, max_trim, long_runs):
            nrec = levels = 0
            if status is None:
                F, G = up[a - k + 1:a], up[q:q + k - 1]
                assert len(F) == k - 1 and len(G) == k - 1 and all(ch in ACGT for ch in F + G)
                lv.append([])
                status, levels, found = search(F, G, k, count, thre, max_len, lv[-1]) if search is search_site else search(F, G, k, count, thre, max_len)
                nrec = len(found)
                recs += [(si, a, q - a, t, y, rmin, amin) for t, y, amin in found]
            sites.append((si, a, q, kind, status, nrec, levels, tl, tr, rmin))
    if stats is not None:
        stats["levels"] = lv
    return _finish(len(seqs), sites, recs)


def restate_gap_search(seqs, k, count, thre, max_len, sites, stats=None):
    """the search alone on explicit sites [(seq, a, q, ref_min)] in (seq, a) order: (counts, sites, records) as restate_gaps gives them"""
    out, recs, lv = [], [], []
    for si, a, q, rmin in sites:
        b = as_bytes(seqs[si])
        assert k - 1 <= a <= q <= len(b) - (k - 1)
        F, G = b[a - k + 1:a].upper(), b[q:q + k - 1].upper()
        if not all(ch in ACGT for ch in F + G):
            out.append((si, a, q, "explicit", "skipped", 0, 0, 0, 0, rmin))
            continue
        lv.append([])
        status, levels, found = search_site(F, G, k, count, thre, max_len, lv[-1])
        recs += [(si, a, q - a, t, y, rmin, amin) for t, y, amin in found]
        out.append((si, a, q, "explicit", status, len(found), levels, 0, 0, rmin))
    if stats is not None:
        stats["levels"] = lv
    return _finish(len(seqs), out, recs)


# ---- the restatement against its plain form ------------------------------------------------------------------------------------------
def tiny_fuzz(k, seed=911):
    """reads that hold g three times and a second haplotype twice; contigs made of g with N runs, runs of other non-base bytes, dirty
    ends, lower case, gaps at the edges, short ones"""
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, 200)
    g2 = substitute(g, [60, 130])
    c1 = bytearray(g)
    c1[40:43] = b"NNN"                                            # three bases for three
    c1[57:62] = b"N"                                              # one N for five bases, a het site among them
    c1[100:100] = b"nn"                                           # an insertion of two: the fill is empty
    c2 = bytearray(substitute(g, [80 - 2, 150 + k + 1]))          # dirty ends on either side
    c2[80:90] = b"RRR"
    c2[140:150] = b"-" * 12
    c2[20:30] = bytes(c2[20:30]).lower()
    c3 = bytearray(g)
    c3[2] = ord("N")                                              # edge on the left
    c3[-3] = ord("N")                                             # ... and on the right
    c3[90:95] = b"NN"
    c4 = bytearray(g[:120])
    c4[50:52] = b"NN"
    c4[52 + k - 2:52 + k] = b"NN"                                 # k - 2 bases between two N runs: one site
    return [g] * 3 + [g2] * 2, [bytes(c1), bytes(c2), bytes(c3), bytes(c4), g[:k - 1], b"", b"N" * (k + 2), g[10:10 + 2 * k]]


def test_the_restatement_agrees_with_its_plain_form():
    seen = dict(records=0, searched=0, edge=0, ragged=0, limit=0, complex=0, dead=0)
    for k in (4, 5, 6):
        reads, seqs = tiny_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        for thre, max_len, max_trim, long_runs in ((1, 0, k, False), (1, 6, k, True), (2, 3, 1, False), (2, 5, k, True), (3, 4, 0, True), (4, 6, k, True)):
            got = restate_gaps(seqs, k, count, thre, max_len, max_trim, long_runs)
            assert got == restate_gaps(seqs, k, count, thre, max_len, max_trim, long_runs, search=search_site_plain), (k, thre, max_len)
            for c in got[0]:
                seen["searched"] += c[1]
                seen["records"] += c[4]
                seen["edge"] += c[5]
                seen["ragged"] += c[6]
                seen["limit"] += c[7]
                seen["complex"] += c[8]
                assert c[0] == c[1] + c[5] + c[6] and c[3] <= c[2] <= c[1] and c[2] <= c[4]
            seen["dead"] += sum(s[4] == "dead" for s in got[1])
    assert seen["records"] > 40 and seen["searched"] > 40 and min(seen.values()) > 0, seen


# ---- planted gaps --------------------------------------------------------------------------------------------------------------------
def fill_lengths(k):
    return sorted({0, 1, k - 2, k - 1, k, 63, 64, 65, 127, 128, 129})


def planted_fills(k, lengths=None, seed=505, n_runs=None):
    """(truth, contig, [(a, n_N, L, p)]): one contig in which, 4k bases apart, the L bases truth[p .. p+L) are an N run of another length
    (10 Ns for L = 129, 200 Ns for L = 1), starting at a"""
    rng = np.random.default_rng(seed + k)
    lengths = fill_lengths(k) if lengths is None else lengths
    truth = rand_bases(rng, 4 * k * (len(lengths) + 1) + sum(lengths))
    contig, plants, p = bytearray(), [], 0
    for i, L in enumerate(lengths):
        contig += truth[p:p + 4 * k]
        p += 4 * k
        nn = (n_runs or {}).get(L, {129: 10, 1: 200}.get(L, L + 3 + i))
        plants.append((len(contig), nn, L, p))
        contig += b"N" * nn
        p += L
    contig += truth[p:]
    assert p + 4 * k == len(truth)
    return truth, bytes(contig), plants


@pytest.mark.parametrize("k", [21, 32, 64])
def test_planted_fills(k):
    """five copies of a random truth, thre 3: a planted fill of length L is listed once, equal to the truth, and the search ends dead at
    level L + k - 1, where the string holds the whole right flank"""
    truth, contig, plants = planted_fills(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    st = {}
    counts, sites, recs = restate_gaps([contig], k, count, 3, 200, k, False, st)
    assert recs == [(0, a, nn, L, truth[p:p + L].decode(), 0, 5) for a, nn, L, p in plants]
    assert sites == [(0, a, a + nn, "gap", "dead", 1, L + k - 1, 0, 0, 0) for a, nn, L, p in plants]
    assert counts == [(len(plants), len(plants), len(plants), len(plants), len(plants), 0, 0, 0, 0)]
    assert all(set(lv) == {1} for lv in st["levels"])
    from jasper_amd import gaps
    assert gaps.fill_sequences([contig], sites, recs) == [truth]


@pytest.mark.parametrize("k", [21, 32, 64])
def test_the_limit_on_either_side_of_a_fill(k):
    """max_len L - 1: no record, limit.  L: one record, the truth, limit.  Large: the same record, dead at level L + k - 1."""
    for L in (0, 1, k - 2, k - 1, k, 63, 64, 65, 129, 500):
        truth, contig, plants = planted_fills(k, [L], seed=77 + L)
        (a, nn, _, p), = plants
        count = dict_counter(kmer_dict([truth] * 5, k))
        rec = (0, a, nn, L, truth[p:p + L].decode(), 0, 5)
        if L:
            assert restate_gaps([contig], k, count, 3, L - 1, k, False)[1:] == ([(0, a, a + nn, "gap", "limit", 0, L - 1, 0, 0, 0)], [])
        assert restate_gaps([contig], k, count, 3, L, k, False)[1:] == ([(0, a, a + nn, "gap", "limit", 1, L, 0, 0, 0)], [rec])
        assert restate_gaps([contig], k, count, 3, L + 2 * k, k, False)[1:] == ([(0, a, a + nn, "gap", "dead", 1, L + k - 1, 0, 0, 0)], [rec])


def repeat_workload(unit, copies, k=21, seed=31):
    """(reads, contig, a): random flanks around `unit` x copies; in the contig three bytes in the middle of the repeat are Ns"""
    rng = np.random.default_rng(seed)
    left, right = rand_bases(rng, 3 * k), rand_bases(rng, 3 * k)
    truth = left + unit * copies + right
    a = len(left) + (len(unit) * copies) // 2
    return [truth] * 5, truth[:a] + b"NNN" + truth[a + 3:], a


def test_a_tandem_repeat_is_cut_at_k_minus_1():
    """a site inside (ACG)x40 at k = 21: a fill of 3 restores the truth, but 0, 6, .., 18 rejoin as well; at 20 bases the string in phase
    holds the whole right flank and leaves, and what walked out of the repeat ends with the reads"""
    reads, contig, a = repeat_workload(b"ACG", 40)
    count = dict_counter(kmer_dict(reads, 21))
    counts, sites, recs = restate_gaps([contig], 21, count, 3, 200, 21, False)
    assert [r[3] for r in recs] == [0, 3, 6, 9, 12, 15, 18]
    assert [r[4] for r in recs] == [(contig[a - 3:a] * 7)[:t].decode() for t in range(0, 21, 3)]
    assert sites == [(0, a, a + 3, "gap", "dead", 7, sites[0][6], 0, 0, 0)] and counts == [(1, 1, 1, 0, 7, 0, 0, 0, 0)]
    from jasper_amd import gaps
    assert gaps.fill_sequences([contig], sites, recs) == [contig]                 # seven records: not unique, not filled


def test_a_homopolymer_reaches_the_record_cap():
    """a site inside Ax60 at k = 21: the lengths 0 .. 15 are listed, the seventeenth record at level 16 makes the site complex"""
    reads, contig, a = repeat_workload(b"A", 60)
    count = dict_counter(kmer_dict(reads, 21))
    counts, sites, recs = restate_gaps([contig], 21, count, 3, 200, 21, False)
    assert [(r[3], r[4]) for r in recs] == [(t, "A" * t) for t in range(16)]
    assert sites == [(0, a, a + 3, "gap", "complex", 16, 16, 0, 0, 0)] and counts == [(1, 1, 1, 0, 16, 0, 0, 0, 1)]


# ---- site rules ------------------------------------------------------------------------------------------------------------------------
def site_cases(k=21, seed=64):
    """[(what, contig, max_trim, long_runs, [(a, q, kind, status, trim_left, trim_right)])] on one truth of 40k bases, five copies of
    which are the reads (thre 3).  The expected sites are written out by hand from the rules."""
    rng = np.random.default_rng(seed + k)
    truth = rand_bases(rng, 40 * k)

    def with_bytes(pairs, subs=()):
        c = bytearray(substitute(truth, subs))
        for p, bs in pairs:
            c[p:p + len(bs)] = bs
        return bytes(c)

    p = 10 * k
    cases = [
        ("two N runs k - 1 bases apart are one site", with_bytes([(p, b"NN"), (p + 2 + k - 1, b"NNN")]), k, False, [(p, p + 2 + k - 1 + 3, "gap", None, 0, 0)]),
        ("two N runs with one solid window between are two sites", with_bytes([(p, b"NN"), (p + 2 + k, b"NNN")]), k, False,
         [(p, p + 2, "gap", None, 0, 0), (p + 2 + k, p + 2 + k + 3, "gap", None, 0, 0)]),
        ("a substitution 3 bases before an N run moves a left", with_bytes([(p, b"NNNN")], [p - 4]), 4, False, [(p - 4, p + 4, "gap", None, 4, 0)]),
        ("... and with max_trim one less it is ragged", with_bytes([(p, b"NNNN")], [p - 4]), 3, False, [(p - 4, p + 4, "gap", "ragged", 4, 0)]),
        ("a substitution 2 bases after an N run moves q right", with_bytes([(p, b"NNNN")], [p + 6]), 3, False, [(p, p + 7, "gap", None, 0, 3)]),
        ("... ragged on the right", with_bytes([(p, b"NNNN")], [p + 6]), 2, False, [(p, p + 7, "gap", "ragged", 0, 3)]),
        ("a gap less than k - 1 from the left end is edge", with_bytes([(k - 2, b"N")]), k, False, [(k - 1, k - 1, "gap", "edge", 0, 0)]),
        ("with k - 1 bases before it it is edge still: window 0 is the solid window it lacks", with_bytes([(k - 1, b"N")]), k, False, [(k - 1, k, "gap", "edge", 0, 0)]),
        ("a gap with k bases before it is searched", with_bytes([(k, b"N")]), k, False, [(k, k + 1, "gap", None, 0, 0)]),
        ("a gap less than k - 1 from the right end is edge", with_bytes([(40 * k - k + 1, b"N")]), k, False, [(40 * k - k + 1, 40 * k - k + 1, "gap", "edge", 0, 0)]),
        ("with k - 1 bases after it it is edge still", with_bytes([(40 * k - k, b"N")]), k, False, [(40 * k - k, 40 * k - k + 1, "gap", "edge", 0, 0)]),
        ("a gap with k bases after it is searched", with_bytes([(40 * k - k - 1, b"N")]), k, False, [(40 * k - k - 1, 40 * k - k, "gap", None, 0, 0)]),
        ("lower-case flanks", with_bytes([(p - 30, truth[p - 30:p].lower()), (p, b"NNN"), (p + 3, truth[p + 3:p + 40].lower())]), k, False, [(p, p + 3, "gap", None, 0, 0)]),
        ("R, - and n are non-base bytes", with_bytes([(p, b"R"), (p + 3 * k, b"-"), (p + 6 * k, b"n")]), k, False,
         [(p, p + 1, "gap", None, 0, 0), (p + 3 * k, p + 3 * k + 1, "gap", None, 0, 0), (p + 6 * k, p + 6 * k + 1, "gap", None, 0, 0)]),
        ("an unreliable run of R = 64 is no site", with_bytes([], [p, p + 16, p + 32, p + 48, p + 63]), k, True, []),
        ("... of R = 65 is a run site with long_runs", with_bytes([], [p, p + 16, p + 32, p + 48, p + 64]), k, True, [(p, p + 65, "run", None, 0, 0)]),
        ("... and none without", with_bytes([], [p, p + 16, p + 32, p + 48, p + 64]), k, False, []),
    ]
    return truth, cases


@pytest.mark.parametrize("k", [21, 32])
def test_site_rules(k):
    truth, cases = site_cases(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    for what, contig, max_trim, long_runs, want in cases:
        got = find_sites(contig, k, count, 3, max_trim, long_runs)
        if "edge" in what:                                    # (a and q of an edge site follow from u0 and u1 alone: only kind and status are stated)
            assert [(s[2], s[3], s[4], s[5]) for s in got] == [(w[2], w[3], w[4], w[5]) for w in want], what
        else:
            assert [s[:6] for s in got] == want, what
    assert find_sites(truth[:k - 1], k, count, 3, k, True) == [] and find_sites(b"N" * (k - 1), k, count, 3, k, True) == [] and find_sites(b"", k, count, 3, k, True) == []
    # the dirty end is part of the fill: with the trim allowed the one record restores the truth
    _, contig, max_trim, _, _ = [c for c in cases if "moves a left" in c[0]][0]
    counts, sites, recs = restate_gaps([contig], k, count, 3, 100, max_trim, False)
    from jasper_amd import gaps
    assert counts == [(1, 1, 1, 1, 1, 0, 0, 0, 0)] and recs[0][2:5] == (8, 8, truth[10 * k - 4:10 * k + 4].decode()) and recs[0][5] == 0
    assert gaps.fill_sequences([contig], sites, recs) == [truth]
    # the run site's fill is the truth as well, and its ref_min is the run's
    _, contig, _, _, _ = [c for c in cases if "R = 65" in c[0]][0]
    counts, sites, recs = restate_gaps([contig], k, count, 3, 100, k, True)
    assert counts == [(1, 1, 1, 1, 1, 0, 0, 0, 0)] and gaps.fill_sequences([contig], sites, recs) == [truth] and sites[0][3] == "run"


# ---- gaps_host.hpp under sanitizers ----------------------------------------------------------------------------------------------------
def test_host_check_program_under_sanitizers(tmp_path):
    """tools/gaps_host_check.cpp: jasper_amd/csrc/gaps_host.hpp as a stand-alone program built with -fsanitize=address,undefined.  It
    makes the sites of every site case and of the tiny fuzz from the two run lists, as the library does, and they are the restatement's;
    then it runs its own checks of the refusals."""
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "gaps_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "gaps_host_check.cpp"), "-o", exe])
    kinds, status = {"gap": 1, "run": 2}, {None: 0, "edge": 4, "ragged": 5}
    work = []
    for k in (21, 32):
        truth, cases = site_cases(k)
        count = dict_counter(kmer_dict([truth] * 5, k))
        for _, contig, max_trim, long_runs, _ in cases:
            work.append((k, [contig, truth[:k - 1], b"", b"N" * (k + 5)], count, 3, max_trim, long_runs))
    for k in (4, 6):
        reads, seqs = tiny_fuzz(k)
        for thre, max_trim, long_runs in ((1, k, True), (3, 0, False), (4, 2, True)):
            work.append((k, seqs, dict_counter(kmer_dict(reads, k)), thre, max_trim, long_runs))
    n_sites = 0
    for i, (k, seqs, count, thre, max_trim, long_runs) in enumerate(work):
        wcs = [window_counts(s, k, count) for s in seqs]
        unrel = restate_runs(wcs, thre)[1]
        inval = restate_runs([[0 if c is None else 1 for c in wc] for wc in wcs], 1)[1]       # the same run finder on "this window has no k-mer"
        path = tmp_path / ("case%d.txt" % i)
        path.write_text(" ".join(str(x) for x in [k, len(seqs), max_trim, int(long_runs)] + [len(s) for s in seqs] + [len(unrel)] +
                                 [x for r in unrel for x in (r[0], r[1], r[2], r[4])] + [len(inval)] + [x for r in inval for x in (r[0], r[1], r[2])]))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr)
        lines = r.stdout.split("\n")
        assert lines[-2:] == ["ok", ""]
        want = ["%d %d %d %d %d %d %d %d" % (si, a, q, kinds[kind], status[st], tl, tr, rmin)
                for si, s in enumerate(seqs) for a, q, kind, st, tl, tr, rmin in find_sites(s, k, count, thre, max_trim, long_runs)]
        assert lines[:-2] == want, i
        n_sites += len(want)
    assert n_sites > 60


# ---- writers ---------------------------------------------------------------------------------------------------------------------------
NAMES = ["c1", "c2"]
# (seq, a, q, kind, status, n_records, levels, trim_left, trim_right, ref_min)
SITES = [(0, 10, 14, "gap", "dead", 1, 25, 0, 0, 0), (0, 30, 33, "gap", "dead", 2, 40, 1, 2, 1), (0, 50, 50, "gap", "edge", 0, 0, 0, 0, 0),
         (1, 5, 9, "gap", "complex", 1, 7, 0, 0, 0), (1, 20, 90, "run", "limit", 0, 100, 0, 0, 2), (1, 95, 97, "gap", "dead", 1, 20, 0, 0, 0),
         (1, 99, 103, "gap", "ragged", 0, 0, 30, 0, 0)]
# (seq, pos, ref_len, len, y, ref_min, alt_min)
RECS = [(0, 10, 4, 6, "ACGTAC", 0, 7), (0, 30, 3, 2, "GG", 1, 5), (0, 30, 3, 2, "GT", 1, 4), (1, 5, 4, 1, "T", 0, 9), (1, 95, 2, 0, "", 0, 3)]


def test_tsv_bed_fills_and_log_texts():
    from jasper_amd import gaps
    c0, c1 = (3, 2, 2, 1, 3, 1, 0, 0, 0), (4, 3, 2, 1, 2, 0, 1, 1, 1)
    stages = [("before", [60, 120], [c0, c1]), ("after", [62, 0], [c0, None])]
    assert gaps.gaps_tsv_text(NAMES, stages) == (
        "#contig\tstage\tlength\tsites\tsearched\tbridged\tunique\trecords\tedge\tragged\tlimit\tcomplex\n"
        "c1\tbefore\t60\t3\t2\t2\t1\t3\t1\t0\t0\t0\nc1\tafter\t62\t3\t2\t2\t1\t3\t1\t0\t0\t0\n"
        "c2\tbefore\t120\t4\t3\t2\t1\t2\t0\t1\t1\t1\nc2\tafter\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n"
        "*\tbefore\t180\t7\t5\t4\t2\t5\t1\t1\t1\t1\n*\tafter\t62\t3\t2\t2\t1\t3\t1\t0\t0\t0\n")
    assert gaps.bed_text(NAMES, SITES, RECS) == (
        "c1\t10\t14\tgap\tdead\t1\t0\t0\t6\t7\n"
        "c1\t30\t33\tgap\tdead\t2\t1\t2\t.\t.\n"
        "c1\t50\t50\tgap\tedge\t0\t0\t0\t.\t.\n"
        "c2\t5\t9\tgap\tcomplex\t1\t0\t0\t.\t.\n"
        "c2\t20\t90\trun\tlimit\t0\t0\t0\t.\t.\n"
        "c2\t95\t97\tgap\tdead\t1\t0\t0\t0\t3\n"
        "c2\t99\t103\tgap\tragged\t0\t30\t0\t.\t.\n")
    assert gaps.fills_tsv_text(NAMES, RECS) == (
        "#contig\tpos\tref_len\tlen\tref_min\talt_min\tfill\n"
        "c1\t10\t4\t6\t0\t7\tACGTAC\nc1\t30\t3\t2\t1\t5\tGG\nc1\t30\t3\t2\t1\t4\tGT\nc2\t5\t4\t1\t0\t9\tT\nc2\t95\t2\t0\t0\t3\t.\n")
    assert gaps.fills_tsv_text(NAMES, []) == "#contig\tpos\tref_len\tlen\tref_min\talt_min\tfill\n" and gaps.bed_text(NAMES, [], []) == ""
    assert gaps.stage_log_text([c0, c1]) == "7 sites, 5 searched, 4 bridged, 2 unique, 5 records, 1 edge, 1 ragged, 1 limit, 1 complex"
    assert gaps.log_text([c0, c1], [c0, None]) == ("Gap scan: before polishing 7 sites, 5 searched, 4 bridged, 2 unique, 5 records, 1 edge, 1 ragged, 1 limit, 1 complex; "
                                                  "after polishing 3 sites, 2 searched, 2 bridged, 1 unique, 3 records, 1 edge, 0 ragged, 0 limit, 0 complex")


def test_fill_sequences_applies_unique_fills_only():
    from jasper_amd import gaps
    s0 = "acgtacgtacNNNNgtacgtacgtacgtacNNNacgtacgtacgtacgtacgtacgtacgt"
    s1 = "ttttcNNNNa" + "c" * 85 + "NNg" + "aNNNNtt"
    got = gaps.fill_sequences([s0, s1], SITES, RECS)
    assert got[0] == s0[:10] + "ACGTAC" + s0[14:]                  # the site with two records and the edge site stay
    assert got[1] == s1[:95] + s1[97:]                             # the complex site stays although it has one record; the empty fill is a deletion
    assert gaps.fill_sequences([s0.encode(), s1.encode()], SITES, RECS) == [g.encode() for g in got]
    assert gaps.fill_sequences([s0, s1], [], []) == [s0, s1]
    # from the structured arrays of a GapScan: the same
    from jasper_amd.table import GAP_FILL_DTYPE, GAP_SITE_DTYPE, GapScan
    kinds, status = {"explicit": 0, "gap": 1, "run": 2}, {"dead": 1, "limit": 2, "complex": 3, "edge": 4, "ragged": 5, "skipped": 6}
    sites = np.zeros(len(SITES), dtype=GAP_SITE_DTYPE)
    for i, (seq, a, q, kind, st, nrec, lv, tl, tr, rmin) in enumerate(SITES):
        sites[i] = (a, q, seq, rmin, nrec, lv, tl, tr, kinds[kind], status[st], [0] * 6)
    recs = np.zeros(len(RECS), dtype=GAP_FILL_DTYPE)
    pool = b""
    for i, (seq, pos, rlen, ln, y, rmin, amin) in enumerate(RECS):
        recs[i] = (pos, len(pool), seq, rlen, ln, amin)
        pool += y.encode()
    gs = GapScan([], sites, recs, pool, None, 0.0, 0.0, 0.0, 0, False)
    assert gs.record_tuples() == RECS and gs.site_tuples() == SITES
    assert gaps.fill_sequences([s0, s1], gs.sites, gs.record_tuples()) == got and gaps.bed_text(NAMES, gs.sites, gs.record_tuples()) == gaps.bed_text(NAMES, SITES, RECS)
    assert gs == GapScan([], sites.copy(), recs.copy(), pool, None, 1.0, 1.0, 1.0, 5, True) and gs != GapScan([], sites, recs, pool[:-1] + b"A", None, 0.0, 0.0, 0.0, 0, False)


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def _run(module, args, cwd):
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)


BAD_FLAGS = [(["--gap-max-len", "5"], "--gap-max-len is an option of the gap scan: give --gaps as well"),
             (["--gap-max-trim", "5"], "--gap-max-trim is an option of the gap scan: give --gaps as well"),
             (["--gap-long-runs"], "--gap-long-runs is an option of the gap scan: give --gaps as well"),
             (["--gaps", "--gap-max-len", "4097"], "--gap-max-len takes an integer from 0 to 4096; it is 4097"),
             (["--gaps", "--gap-max-len", "-1"], "--gap-max-len takes an integer from 0 to 4096; it is -1"),
             (["--gaps", "--gap-max-len", "x"], "--gap-max-len takes an integer from 0 to 4096; it is x"),
             (["--gaps", "--gap-max-trim", "1001"], "--gap-max-trim takes an integer from 0 to 1000; it is 1001"),
             (["--gaps", "--gap-max-trim", "1.5"], "--gap-max-trim takes an integer from 0 to 1000; it is 1.5")]


@pytest.mark.parametrize("module", ["jasper_amd.cli", "jasper_amd.kmerqc"])
@pytest.mark.parametrize("bad,msg", BAD_FLAGS)
def test_a_bad_flag_ends_the_run(module, bad, msg, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "r.fa"
    fq.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    args = ["-a", str(fa), "-r", str(fq), "-k", "5"] + bad + (["--threshold", "1"] if module.endswith("kmerqc") else [])
    r = _run(module, args, tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert msg in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


def test_gaps_fill_is_the_drivers(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    r = _run("jasper_amd.cli", ["-a", str(fa), "-r", str(fa), "-k", "5", "--gaps-fill"], tmp_path)
    assert r.returncode == 1 and "--gaps-fill is an option of the gap scan: give --gaps as well" in r.stdout + r.stderr
    r = _run("jasper_amd.kmerqc", ["-a", str(fa), "-r", str(fa), "-k", "5", "--gaps", "--gaps-fill", "--threshold", "1"], tmp_path)
    assert r.returncode == 1 and "Unknown option --gaps-fill" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name != "a.fa"] == []


def test_threshold_zero_ends_kmerqc(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    r = _run("jasper_amd.kmerqc", ["-a", str(fa), "-r", str(fa), "-k", "5", "--gaps", "--threshold", "0"], tmp_path)
    assert r.returncode == 1 and "--gaps needs a threshold of at least 1; --threshold 0 was given" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name != "a.fa"] == []


def test_threshold_zero_ends_the_driver_and_the_flags_parse(capsys):
    """the driver takes its threshold from threshold.txt after the polishing: its scan function refuses 0 before it touches the table"""
    from jasper_amd import cli, kmerqc
    with pytest.raises(SystemExit) as e:
        cli.scan_gaps(None, [(">c", "ACGT")], 0, 1000)
    assert e.value.code == 1
    out = capsys.readouterr()
    assert "--gaps needs a threshold for unreliable kmers of at least 1; it is 0" in out.out + out.err
    assert cli.gap_flags(True, None, None) == (1000, None) and cli.gap_flags(True, "0", "0", True, True) == (0, 0) and cli.gap_flags(True, "4096", "1000") == (4096, 1000)
    assert cli.gap_flags(False, None, None) == (None, None)
    o = cli.parse_args(["-a", "x/asm.fa", "--gaps", "--gap-max-len", "50", "--gap-max-trim", "7", "--gap-long-runs", "--gaps-fill"])
    assert o.gaps and o.gap_long_runs and o.gaps_fill and (o.gap_max_len, o.gap_max_trim) == ("50", "7")
    o = cli.parse_args(["-a", "x/asm.fa"])
    assert not o.gaps and not o.gap_long_runs and not o.gaps_fill and o.gap_max_len is None
    a = kmerqc.parse_args(["-a", "asm.fa", "-r", "r.fq", "--gaps", "--gap-long-runs", "--gap-max-len", "9"])
    assert a["gaps"] and a["gap_long_runs"] and a["gap_max_len"] == "9" and not a["gaps_fill"]
