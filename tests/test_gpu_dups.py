"""GPU: the duplication map (KmerTable.dup_map / dup_map_device, jasper_dup_map) against a restatement of its semantics fed by Python
dicts: canonical k-mer -> the (global position, strand bit) of its occurrences over the scanned sequences, and canonical k-mer -> count
in the reads.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): window i of sequence s is valid iff all k bytes are ACGTacgt; its strand bit is 1 iff rc < fwd; its
global position is offsets[s] + i, encoded as 2 * position + strand.  For a == 2 the k-mer's slot holds the smallest and the largest
encoded position seen in the scanned sequences; the window is two-copy iff those are two different positions and one is its own (the
other is its mate), else unplaced; a >= 3 is multi.  Orientation `+` iff the two strand bits are equal.  deficit iff two-copy, c >= thre
and (2c + peak) div (2 peak) < 2.  A run is a maximal range of consecutive two-copy windows of one orientation with colinear mates:
(seq, start, n_kmers, mate_seq, mate_start (leftmost), strand, sum_reads, n_deficit).

The forced-retry path (more partial runs than the first list holds) is not exercised here: it would need some 70 000 separate two-copy
runs; the repeat itself is the shared run_counted's, which tests/test_gpu_copies.py covers."""
import bisect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
TILE = 4096
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def revcomp(b):
    return bytes(b).upper().translate(_COMP)[::-1]


def rand(rng, n):
    return _BASES[rng.integers(0, 4, n)].tobytes()


def other(base):
    """a base that differs from the byte given (a run must end where the test says it ends)"""
    return b"ACGT"[(b"ACGT".index(bytes([base]).upper()) + 1) % 4:][:1]


def canon(km):
    rc = km.translate(_COMP)[::-1]
    return (rc, 1) if rc < km else (km, 0)


def windows(seq, k):
    """per window: None (not valid) or (canonical k-mer, strand bit)"""
    b = bytes(seq)
    n = len(b)
    pre = [0] * (n + 1)
    for i, ch in enumerate(b):
        pre[i + 1] = pre[i] + (0 if ch in b"ACGTacgt" else 1)
    up = b.upper()
    return [canon(up[i:i + k]) if pre[i + k] == pre[i] else None for i in range(max(0, n - k + 1))]


def count_dict(seqs_mult, k):
    """canonical k-mer -> occurrences over [(sequence, multiplicity)]"""
    d = {}
    for s, mult in seqs_mult:
        for w in windows(s, k):
            if w is not None:
                d[w[0]] = d.get(w[0], 0) + mult
    return d


def restate(seqs, k, rd, thre, peak, ad=None):
    """(counts, runs) of the semantics above; ad = A's counts when A is NOT counted from `seqs` (default: the length of the position list)"""
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    wins = [windows(s, k) for s in seqs]
    places = {}
    for si, ws in enumerate(wins):
        for i, w in enumerate(ws):
            if w is not None:
                places.setdefault(w[0], []).append(2 * (offs[si] + i) + w[1])
    counts, runs = [], []
    for si, ws in enumerate(wins):
        valid = two = de = multi = unplaced = sr = 0
        cur = prev = None               # prev: (orientation, mate position) of the window before, if it is two-copy
        for i, w in enumerate(ws):
            key = None
            if w is not None:
                valid += 1
                a = len(places[w[0]]) if ad is None else ad.get(w[0], 0)
                c = min(rd.get(w[0], 0), U32)
                if a >= 3:
                    multi += 1
                elif a == 2:
                    p = places[w[0]]
                    own = 2 * (offs[si] + i) + w[1]
                    mn, mx = min(p), max(p)
                    if mn != mx and own in (mn, mx):
                        mate = mx if own == mn else mn
                        key = ((mate ^ own) & 1, mate >> 1)
                    else:
                        unplaced += 1
            cont = key is not None and prev is not None and key[0] == prev[0] and key[1] == prev[1] + (-1 if key[0] else 1)
            if cur is not None and not cont:
                runs.append(cur)
                cur = None
            if key is not None:
                two += 1
                sr += c
                d = c >= thre and (2 * c + peak) // (2 * peak) < 2
                de += d
                if cur is None:
                    cur = [si, i, 0, key[1], key[1], key[0], 0, 0]      # [3]: the leftmost mate so far, a global position
                cur[2] += 1
                cur[3] = min(cur[3], key[1])
                cur[6] += c
                cur[7] += d
            prev = key
        if cur is not None:
            runs.append(cur)
        counts.append((len(ws), valid, two, de, multi, unplaced, sr))
    out = []
    for si, start, n, left, _, strand, sr, nd in runs:
        ms = bisect.bisect_right(offs, left) - 1
        while len(seqs[ms]) == 0:
            ms -= 1
        out.append((si, start, n, ms, left - offs[ms], strand, sr, nd))
    return counts, out


def mirror_closed(runs):
    """the runs as a multiset are closed under (seq, start) <-> (mate_seq, mate_start) with the same strand and n_kmers"""
    a = sorted((r[0], r[1], r[3], r[4], r[5], r[2]) for r in runs)
    b = sorted((r[3], r[4], r[0], r[1], r[5], r[2]) for r in runs)
    return a == b


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


def tables(KT, k, seqs, reads, asm_seqs=None):
    """R counted from the reads [(sequence, multiplicity)], A from the scanned sequences joined by a separator byte"""
    r = KT(k, min_slots=1 << 16)
    r.count_bases(b"N".join(s for s, mult in reads for _ in range(mult)))
    a = KT(k, min_slots=1 << 16)
    a.count_bases(b"N".join(bytes(s) for s in (seqs if asm_seqs is None else asm_seqs)))
    return r, a


def run_case(KT, seqs, k, reads=None, thre=1, peak=4, asm_seqs=None, what=""):
    """dup_map of the case against the restatement; -> (DupMap, want_counts, want_runs)"""
    reads = [(s, 2) for s in seqs] if reads is None else reads
    r, a = tables(KT, k, seqs, reads, asm_seqs)
    try:
        rep = r.dup_map(a, seqs, thre, peak)
    finally:
        r.close()
        a.close()
    rd = count_dict(reads, k)
    ad = None if asm_seqs is None else count_dict([(s, 1) for s in asm_seqs], k)
    want_counts, want_runs = restate(seqs, k, rd, thre, peak, ad)
    got = rep.run_tuples()
    print(what, [tuple(sum(c[i] for c in want_counts) for i in range(7))], len(want_runs), len(got))
    assert rep.counts == want_counts, what
    assert len(got) == len(want_runs), (what, len(got), len(want_runs))
    assert got == want_runs, what
    assert all(int(p) == 0 for p in rep.runs["pad"])
    assert mirror_closed(got), what
    if asm_seqs is None:
        assert all(c[5] == 0 for c in rep.counts), "unplaced windows with the matching A"
    assert rep.seconds[0] > 0 and rep.seconds[1] > 0 and not rep.retried
    return rep, want_counts, want_runs


def planted(rng, n, at, seg):
    """a random sequence of n bytes with seg at `at`, the bytes next to it chosen by the caller afterwards"""
    s = bytearray(rand(rng, n))
    s[at:at + len(seg)] = seg
    return s


def isolate(x, at, n, y, yat, minus=False):
    """make the bytes next to x[at:at+n) differ from what lies next to its copy y[yat:yat+n), so that the run is exactly the copy"""
    if minus:
        x[at - 1:at] = other(revcomp(y[yat + n:yat + n + 1])[0])
        x[at + n:at + n + 1] = other(revcomp(y[yat - 1:yat])[0])
    else:
        x[at - 1:at] = other(y[yat - 1])
        x[at + n:at + n + 1] = other(y[yat + n])


def seam_case(rng, k, minus=False, at=3000, seg_len=3000, n=10_000):
    seg = rand(rng, seg_len)
    x = planted(rng, n, at, seg)
    y = planted(rng, seg_len + 3000, 2000, revcomp(seg) if minus else seg)
    isolate(x, at, seg_len, y, 2000, minus)
    return [bytes(x), bytes(y)], (at, seg_len - k + 1)


@pytest.mark.parametrize("minus", [False, True])
def test_run_across_a_tile_seam(KT, minus):
    k = 21
    seqs, (at, nw) = seam_case(np.random.default_rng(1 + minus), k, minus)
    rep, _, want = run_case(KT, seqs, k, what="seam")
    assert (0, at, nw, 1, 2000, int(minus)) in [r[:6] for r in want] and at < TILE < at + nw


def test_copy_inside_one_sequence(KT):
    k = 21
    rng = np.random.default_rng(3)
    seg = rand(rng, 3000)
    x = planted(rng, 12_000, 2500, seg)
    x[8000:11000] = seg
    isolate(x, 2500, 3000, x, 8000)
    _, _, want = run_case(KT, [bytes(x), rand(rng, 500)], k, what="inside")
    assert [r[:6] for r in want] == [(0, 2500, 3000 - k + 1, 0, 8000, 0), (0, 8000, 3000 - k + 1, 0, 2500, 0)]


def test_runs_that_start_and_end_at_a_tile_seam(KT):
    k = 21
    rng = np.random.default_rng(4)
    s1, s2 = rand(rng, 1500), rand(rng, 1500)
    x1 = planted(rng, 10_000, TILE, s1)                         # first window TILE
    e = TILE - 1 + k - len(s2)                                  # last window TILE - 1
    x2 = planted(rng, 10_000, e, s2)
    y = planted(rng, 6000, 1000, s1)
    y[3500:5000] = s2
    isolate(y, 1000, 1500, x1, TILE)
    isolate(y, 3500, 1500, x2, e)
    _, _, want = run_case(KT, [bytes(x1), bytes(x2), bytes(y)], k, what="at the seam")
    assert [r[:6] for r in want if r[0] == 0] == [(0, TILE, 1500 - k + 1, 2, 1000, 0)]
    assert [r[:6] for r in want if r[0] == 1] == [(1, e, 1500 - k + 1, 2, 3500, 0)] and e + 1500 - k == TILE - 1


def test_run_over_more_than_two_tiles(KT):
    k = 21
    rng = np.random.default_rng(5)
    seg = rand(rng, 10_000)
    x = planted(rng, 12_000, 1000, seg)
    y = bytearray(seg + rand(rng, 700))
    x[11_000:11_001] = other(y[10_000])
    rep, _, want = run_case(KT, [bytes(x), bytes(y)], k, what="three tiles")
    assert (0, 1000, 10_000 - k + 1, 1, 0, 0) in [r[:6] for r in want]      # tile 1 (windows 4096 .. 8191) is absorbed whole


@pytest.mark.parametrize("minus", [False, True])
@pytest.mark.parametrize("switch", [2005, 2000, TILE])
def test_diagonal_switch_without_a_gap(KT, switch, minus):
    """X = P Q, Y holds P, W holds the last k - 1 bases of P and Q: the windows of X inside P pair with Y, the very next ones with W"""
    k = 21
    rng = np.random.default_rng(100 + switch + minus)
    P, Q = rand(rng, 1500), rand(rng, 1500)
    px = switch - (len(P) - k + 1)                              # the first window that leaves P is window `switch`
    x = planted(rng, 10_000, px, P + Q)
    y = planted(rng, 3000, 700, P)
    tail = P[-(k - 1):] + Q
    w = planted(rng, 3000, 600, revcomp(tail) if minus else tail)
    isolate(y, 700, len(P), x, px)
    if minus:                                                   # W must not hold the last k-mer of P as well
        w[600 + len(tail):601 + len(tail)] = other(revcomp(P[-k:-k + 1])[0])
    else:
        w[599:600] = other(P[-k])
    _, _, want = run_case(KT, [bytes(x), bytes(y), bytes(w)], k, what="switch")
    xs = [r for r in want if r[0] == 0]
    first = [r for r in xs if r[1] + r[2] == switch]
    second = [r for r in xs if r[1] == switch]
    assert len(first) == 1 and len(second) == 1, xs
    assert first[0][3] == 1 and first[0][2] == len(P) - k + 1 and first[0][5] == 0
    assert second[0][3] == 2 and second[0][2] >= len(Q) and second[0][5] == int(minus)


def test_substitution_and_deletion(KT):
    k = 21
    rng = np.random.default_rng(7)
    s1, s2 = rand(rng, 2000), bytearray(rand(rng, 2000))
    s2[999:1002] = b"ACG"                                       # (the deleted base differs from both its neighbours)
    s2 = bytes(s2)
    x = planted(rng, 9000, 1000, s1)
    x[5000:7000] = s2
    sub = bytearray(s1)
    sub[1000:1001] = other(s1[1000])
    y = planted(rng, 3000, 500, sub)
    z = planted(rng, 3000, 500, s2[:1000] + s2[1001:])
    isolate(y, 500, 2000, x, 1000)
    x[4999:5000] = other(z[499])
    x[7000:7001] = other(z[500 + 1999])
    rep, counts, want = run_case(KT, [bytes(x), bytes(y), bytes(z)], k, what="sub / del")
    xs = [r[:6] for r in want if r[0] == 0]
    assert len(xs) == 4
    a, b, c, d = xs
    assert a[3] == b[3] == 1 and b[1] - (a[1] + a[2]) == k and b[4] - b[1] == a[4] - a[1]            # one diagonal, k windows apart
    assert c[3] == d[3] == 2 and d[1] > c[1] + c[2] and (d[4] - d[1]) - (c[4] - c[1]) == -1          # neighbouring diagonals
    assert counts[0][4] == 0                                                                         # the windows between have a == 1


def test_invalid_bytes_and_case(KT):
    k = 21
    rng = np.random.default_rng(8)
    s1, s2 = rand(rng, 1500), rand(rng, 1500)
    x = planted(rng, 9000, 3500, s1)                            # (across the seam, too)
    x[6000:7500] = s2
    c1 = bytearray(s1)
    c1[700:701] = b"N"
    y = planted(rng, 5000, 300, c1)
    y[2500:4000] = s2.lower()
    rep, counts, want = run_case(KT, [bytes(x), bytes(y)], k, what="N / case")
    ys = [r[:6] for r in want if r[0] == 1]
    assert len(ys) == 3 and ys[1][1] - (ys[0][1] + ys[0][2]) == k and all(c[4] == 0 for c in counts)
    assert counts[1][0] - counts[1][1] == k
    assert ys[2][1:3] == (2500, 1500 - k + 1) or ys[2][2] >= 1500 - k + 1


def test_counters_multi_and_unplaced(KT):
    k = 21
    rng = np.random.default_rng(9)
    s3, s2 = rand(rng, 800), rand(rng, 900)
    x = planted(rng, 9000, 1000, s3)
    x[4000:4800] = s3
    x[6000:6900] = s2
    y = planted(rng, 4000, 500, s3)
    y[2000:2900] = s2
    isolate(y, 2000, 900, x, 6000)
    seqs = [bytes(x), bytes(y)]
    rep, counts, want = run_case(KT, seqs, k, what="multi")
    assert sum(c[4] for c in counts) >= 3 * (800 - k + 1) and all(r[2] <= 900 + 2 for r in want)
    # an A counted from more than the scanned sequences: one more copy of a unique stretch makes its windows unplaced, one more copy of
    # the two-copy stretch makes them multi
    extra = [seqs[0][7500:8200], s2]
    rep, counts, want = run_case(KT, seqs, k, asm_seqs=seqs + extra, what="unplaced")
    assert counts[0][5] == 700 - k + 1 and counts[1][5] == 0 and all(r[2] <= 2 for r in want)      # (what is left: chance matches next to the three copies)
    assert sum(c[4] for c in counts) >= 3 * (800 - k + 1) + 2 * (900 - k + 1)


def test_deficit(KT):
    k = 21
    rng = np.random.default_rng(10)
    s1, s2 = rand(rng, 1200), rand(rng, 1300)
    x = planted(rng, 9000, 3600, s1)
    x[6000:7300] = s2
    y = planted(rng, 3000, 400, s1)
    z = planted(rng, 3000, 500, s2)
    isolate(y, 400, 1200, x, 3600)
    isolate(z, 500, 1300, x, 6000)
    seqs = [bytes(x), bytes(y), bytes(z)]
    reads = [(seqs[0], 30), (seqs[2], 30)]                       # s1's k-mers: c = 30 = peak; s2's: c = 60 = 2 peak
    rep, counts, want = run_case(KT, seqs, k, reads=reads, thre=3, peak=30, what="deficit")
    by = {r[:2]: r for r in want}
    assert by[(0, 3600)][7] == by[(0, 3600)][2] and by[(0, 3600)][6] == 30 * by[(0, 3600)][2]
    assert by[(0, 6000)][7] == 0 and by[(0, 6000)][6] == 60 * by[(0, 6000)][2]
    assert counts[1][3] == counts[1][2] > 0 and counts[2][3] == 0
    rep, counts, want = run_case(KT, seqs, k, reads=reads, thre=61, peak=30, what="thre above c")
    assert all(c[3] == 0 for c in counts) and all(r[7] == 0 for r in want)


@pytest.mark.parametrize("k", [37, 63])
def test_wide_tables(KT, k):
    seqs, (at, nw) = seam_case(np.random.default_rng(k), k, minus=(k == 63))
    r, a = tables(KT, k, seqs, [(s, 1) for s in seqs])
    wide = [2 * k - (t.info()["slots"].bit_length() - 1) > 53 for t in (r, a)]
    r.close()
    a.close()
    assert all(wide)                                            # (csrc/kmer.hpp: wide_rem)
    _, _, want = run_case(KT, seqs, k, what="wide")
    assert (0, at, nw, 1, 2000, int(k == 63)) in [r_[:6] for r_ in want]


def test_even_k_with_a_palindrome_inside_a_copy(KT):
    k = 22
    rng = np.random.default_rng(11)
    half = rand(rng, 11)
    seg = bytearray(rand(rng, 2000))
    seg[900:922] = half + revcomp(half)
    assert canon(bytes(seg[900:922]))[1] == 0 and revcomp(seg[900:922]) == bytes(seg[900:922])
    x = planted(rng, 9000, 3000, seg)
    y = planted(rng, 4000, 1000, revcomp(seg))
    isolate(x, 3000, 2000, y, 1000, minus=True)
    _, _, want = run_case(KT, [bytes(x), bytes(y)], k, what="palindrome")
    # the palindromic window has strand bit 0 in both copies: its orientation is `+` inside a `-` stretch, and it is a run of its own
    xs = [r[:6] for r in want if r[0] == 0]
    assert (0, 3900, 1, 1, 1000 + 2000 - 922, 0) in xs and len(xs) == 3


def test_two_calls_and_device_text(KT, hip):
    import torch
    k = 21
    seqs, _ = seam_case(np.random.default_rng(12), k)
    seqs = seqs + [b"", b"ACGT", rand(np.random.default_rng(13), 300)]
    r, a = tables(KT, k, seqs, [(s, 3) for s in seqs])
    one = r.dup_map(a, seqs, 2, 3)
    two = r.dup_map(a, seqs, 2, 3)
    assert one == two and len(one.runs) >= 2 and one.run_tuples() == restate(seqs, k, count_dict([(s, 3) for s in seqs], k), 2, 3)[1]
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert r.dup_map_device(a, d, offs, 2, 3) == one
    assert r.dup_map(a, [], 2, 3).counts == [] and r.dup_map(a, [b"ACG"], 2, 3).counts == [(0, 0, 0, 0, 0, 0, 0)]
    r.close()
    a.close()


def test_argument_checks(KT):
    k = 21
    s = rand(np.random.default_rng(14), 500)
    r, a = tables(KT, k, [s], [(s, 1)])
    b = KT(23, min_slots=1 << 16)
    b.count_bases(s)
    with pytest.raises(Exception, match="different k"):
        r.dup_map(b, [s], 1, 4)
    with pytest.raises(Exception, match="same table"):
        r.dup_map(r, [s], 1, 4)
    with pytest.raises(Exception, match="peak must be at least 1"):
        r.dup_map(a, [s], 1, 0)
    with pytest.raises(TypeError):
        r.dup_map(None, [s], 1, 4)
    for t in (r, a, b):
        t.close()
