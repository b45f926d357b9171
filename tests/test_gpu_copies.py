"""GPU: the copy-number scan (KmerTable.copy_report / copy_report_device, jasper_copy_report) against a restatement of its semantics
fed by Python dicts of canonical k-mer strings: the dict of a golden case's dump.txt.gz (printed by the real `jellyfish dump -c`) or
a dict of the reads' canonical k-mers for R, a dict of the assembly's for A.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): window i of a sequence of n bytes exists for 0 <= i <= n-k and is valid iff all k bytes are
ACGTacgt; c = its canonical k-mer's count in R and a = in A, both clamped to 2^32-1; e = (2c + peak) div (2 peak); class excess (1)
iff c >= thre and e > a, deficit (2) iff c >= thre and e < a, else 0; per sequence (windows, valid, excess, deficit, sum_reads,
sum_asm); a run is a maximal range of consecutive windows of one non-zero class: (seq, start, n_kmers, kind, sum_reads, sum_asm)."""
import re

import numpy as np
import pytest

from golden_util import Case, case_names

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
TILE = 4096
EXCESS, DEFICIT = 1, 2
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def kmer_dict(seqs, k):
    """canonical k-mer (bytes) -> occurrences over the sequences: upper-cased, every maximal stretch of >= k ACGT bytes walked"""
    d = {}
    for s in seqs:
        for m in re.finditer(rb"[ACGT]{%d,}" % k, as_bytes(s).upper()):
            t = m.group()
            for i in range(len(t) - k + 1):
                km = t[i:i + k]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                d[key] = d.get(key, 0) + 1
    return d


def dict_counter(d):
    def count(km):
        rc = km.translate(_COMP)[::-1]
        return d.get(km if km < rc else rc, 0)
    return count


def window_counts(seq, k, count):
    """per window: None (not valid) or the clamped count; count(bytes of k upper-case bases) -> int"""
    b = as_bytes(seq)
    n = len(b)
    pre = [0] * (n + 1)
    for i, ch in enumerate(b):
        pre[i + 1] = pre[i] + (0 if ch in b"ACGTacgt" else 1)
    up = b.upper()
    return [min(count(up[i:i + k]), U32) if pre[i + k] == pre[i] else None for i in range(max(0, n - k + 1))]


def window_class(c, a, thre, peak):
    if c < thre:
        return 0
    e = (2 * c + peak) // (2 * peak)
    return EXCESS if e > a else DEFICIT if e < a else 0


def restate(wcs, was, thre, peak):
    """(counts, runs) of the semantics above from the per-window counts in R (wcs) and in A (was) of every sequence"""
    counts, runs = [], []
    for si, (wc, wa) in enumerate(zip(wcs, was)):
        valid = ex = de = sr = sa = 0
        cur = None
        for i, (c, a) in enumerate(zip(wc, wa)):
            cls = 0
            if c is not None:
                valid += 1
                sr += c
                sa += a
                cls = window_class(c, a, thre, peak)
                ex += cls == EXCESS
                de += cls == DEFICIT
            if cur is not None and cur[3] != cls:
                runs.append(tuple(cur))
                cur = None
            if cls:
                if cur is None:
                    cur = [si, i, 0, cls, 0, 0]
                cur[2] += 1
                cur[4] += c
                cur[5] += a
        if cur is not None:
            runs.append(tuple(cur))
        counts.append((len(wc), valid, ex, de, sr, sa))
    return counts, runs


def peak_rule(h, thre):
    """the smallest c in [max(thre, 2), 10000] with the largest h[c]; None when all those bins are 0"""
    best, best_n = None, 0
    for c in range(max(thre, 2), 10001):
        if h[c] > best_n:
            best, best_n = c, h[c]
    return best


def histo_of(d):
    h = [0] * 10002
    for c in d.values():
        if c > 0:
            h[min(c, 10001)] += 1
    return h


def expected(seqs, k, rd, ad, thre, peak):
    cr, ca = dict_counter(rd), dict_counter(ad)
    return restate([window_counts(s, k, cr) for s in seqs], [window_counts(s, k, ca) for s in seqs], thre, peak)


def summary(counts, runs):
    """(windows, valid, excess, deficit, sum_reads, sum_asm, excess runs, deficit runs)"""
    return tuple(sum(c[i] for c in counts) for i in range(6)) + (sum(r[3] == EXCESS for r in runs), sum(r[3] == DEFICIT for r in runs))


def check(rep, want_counts, want_runs, what):
    assert rep.counts == want_counts, what
    got = rep.run_tuples()
    assert len(got) == len(want_runs), (what, len(got), len(want_runs))
    assert got == want_runs, what


def tile_ends_crossed(r):
    """tile ends strictly inside the run: windows i, i+1 both in the run with i+1 a multiple of TILE"""
    return (r[1] + r[2] - 1) // TILE - r[1] // TILE


def asm_table(KT, k, seqs, min_slots=1 << 16):
    """the sequences counted into a table of their own, joined by a separator byte"""
    a = KT(k, min_slots=min_slots)
    a.count_bases(b"N".join(as_bytes(s) for s in seqs))
    return a


def is_wide(t):
    """the low 64 remainder bits of a slot's key are in a second array when 2k - log2(slots) > 53 (csrc/kmer.hpp: wide_rem)"""
    return 2 * t.k - (t.info()["slots"].bit_length() - 1) > 53


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


# peak and (windows, valid, excess, deficit, sum_reads, sum_asm, excess runs, deficit runs), computed on the CPU from the committed dumps
ANCHORS = {"cluster_k25": (30, (5976, 5976, 53, 57, 159913, 5976, 10, 4)),
           "edges_k19": (29, (3013, 2904, 70, 156, 87223, 2998, 7, 12)),
           "rolling_k25": (32, (5275, 5275, 1313, 114, 1193525, 6529, 4, 7)),
           "simple_k63": (24, (3937, 3937, 408, 69, 94292, 3937, 37, 2))}


def golden_expected(c):
    _, seqs = c.batch()
    rd = {key.encode(): v for key, v in c.dump().items()}
    ad = kmer_dict(["N".join(seqs)], c.k)
    peak = peak_rule(histo_of(rd), c.thre)
    return seqs, peak, expected(seqs, c.k, rd, ad, c.thre, peak)


def test_anchored_cases_exist():
    assert set(ANCHORS) <= set(case_names()) and len(case_names()) == 17


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    seqs, peak, (want_counts, want_runs) = golden_expected(c)
    assert peak is not None
    r = KT(c.k, min_slots=1 << 16)
    r.count_text(c.reads_text())
    a = asm_table(KT, c.k, ["N".join(seqs)])
    rep = r.copy_report(a, seqs, c.thre, peak)
    r.close()
    a.close()
    print(name, peak, summary(want_counts, want_runs), summary(rep.counts, rep.run_tuples()))
    check(rep, want_counts, want_runs, name)
    assert sum(r_[3] == DEFICIT for r_ in want_runs) >= 2, "vacuous case"
    if name in ANCHORS:
        assert (peak, summary(want_counts, want_runs)) == ANCHORS[name]
        assert summary(rep.counts, rep.run_tuples()) == ANCHORS[name][1]
    assert rep.seconds > 0 and not rep.retried


def revcomp(b):
    return bytes(b).upper().translate(_COMP)[::-1]


FUZZ_KS = [1, 17, 31, 32, 33, 37, 45, 63, 64]
FUZZ_SEED = {k: 6300 + k for k in FUZZ_KS}


def fuzz_workload(seed, k):
    """(reads, sequences): a 60 000-base genome; a unit U the reads hold three times and the assembly once; a stretch D of the
    genome the assembly holds three times more; a unit W the reads hold four times and the assembly twice, a piece of it joined
    to a piece of D; a unit X the reads hold five times, put behind TILE - 1 windows of the genome; the report test's nuisances;
    the spectra test's homopolymer reads.  The copy numbers are two or more apart, so read noise does not flip a class."""
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    ACGT = synth.ACGT
    genome = synth.make_genome(rng, 60_000)
    U, W, X = (ACGT[rng.integers(0, 4, n)] for n in (9000, 3000, 2500))
    read_genome = np.concatenate([genome] + [U] * 3 + [W] * 4 + [X] * 5)
    reads = synth.make_reads_stream(rng, read_genome, 30, 150, 0.003).tobytes()
    reads += b"N" + b"A" * 20_000 + b"N" + b"C" * (3000 + k - 1) + b"N"      # A^k: 20001 - k times; C^k: 3000 times
    asm = synth.make_assembly(rng, genome, err=2e-3, n_every=9000, n_len=40).copy()
    n = len(asm)
    a0 = int(rng.integers(0, n - 3000))
    asm[a0:a0 + 2000] = np.frombuffer(asm[a0:a0 + 2000].tobytes().lower(), dtype=np.uint8)      # lower case (and 'n' where an N stretch falls)
    for p, ch in zip(rng.integers(0, n, 12).tolist(), b"nRY-*.\n\0\xffxU "):
        asm[p] = ch
    g, u, w, x = genome.tobytes(), U.tobytes(), W.tobytes(), X.tobytes()
    D = g[40_000:49_000]
    seqs = [asm.tobytes(),
            g[30_000:30_300] + u + g[31_000:31_300],                         # collapsed: the reads support 3, the assembly holds 1
            D + b"N" + D.lower() + b"NN" + revcomp(D),                       # duplicated: the reads support 1, the assembly holds 3 or 4
            w,                                                               # 4 against 2 ...
            w[500:2500] + D[3000:5500],                                      # ... joined to 1 against 4 or 5: runs of both kinds side by side
            g[20_000:20_000 + TILE - 2] + (b"C" if x[-1:] != b"C" else b"G") + x,      # 5 against 1, from the first tile's last window on (the base
                                                                             # before X is not the one that precedes X's repeats in the reads)
            b"", g[100:100 + k - 1], g[200:200 + k], g[300:300 + k].lower()]
    if k > 1:
        seqs.append(g[:k - 1] + b"N" + g[k:2 * k - 1])                       # no valid window at all
    for nw in (TILE - 1, TILE, TILE + 1):                                    # exactly one tile of windows +- 1
        seqs.append(g[1000:1000 + nw + k - 1])
    seqs.append(b"C" * (k + 2))                                              # C^k: 3000 in the reads, 3 in the assembly
    for _ in range(300):                                                     # many short sequences
        p = int(rng.integers(0, n - 300))
        seqs.append(asm[p:p + int(rng.integers(0, 260))].tobytes())
    return reads, seqs


def fuzz_expected(k, thres=(0, 1, 3, U32)):
    """the workload of k, its dicts' peak and {thre: (counts, runs)}; the asserts on the restatement that make the test worth running"""
    reads, seqs = fuzz_workload(FUZZ_SEED[k], k)
    assert sum(len(s) for s in seqs) <= 300_000
    rd, ad = kmer_dict([reads], k), kmer_dict(seqs, k)
    peak = peak_rule(histo_of(rd), 3) or 1000        # (k = 1: two keys, both beyond the histogram's last bin -- any peak will do)
    cr, ca = dict_counter(rd), dict_counter(ad)
    wcs, was = [window_counts(s, k, cr) for s in seqs], [window_counts(s, k, ca) for s in seqs]
    want = {t: restate(wcs, was, t, peak) for t in thres}
    if k >= 17:
        runs1 = want[1][1]
        assert any(r[3] == EXCESS and tile_ends_crossed(r) >= 2 for r in runs1), "(a) no excess run across two tile ends"
        assert any(r[3] == DEFICIT and tile_ends_crossed(r) >= 2 for r in runs1), "(b) no deficit run across two tile ends"
        runs0 = want[0][1]
        assert any(p[0] == q[0] and p[3] != q[3] and p[1] + p[2] == q[1] for p, q in zip(runs0, runs0[1:])), "(c) no two runs of different kind touch"
        assert all(any(r[1] % TILE == TILE - 1 and r[2] > 1 for r in want[t][1]) for t in (0, 1, 3)), "(d) no run starts on a tile's last window"
        assert max(max(c for c in wc if c is not None) for wc in wcs if any(c is not None for c in wc)) >= 3000      # counts beyond 2^10
    counts_u, runs_u = want[U32]
    assert runs_u == [] and all(c[2] == 0 and c[3] == 0 for c in counts_u), "(e)"
    assert [(c[0], c[1], c[4], c[5]) for c in counts_u] == [(c[0], c[1], c[4], c[5]) for c in want[1][0]]
    assert sum(c[4] for c in counts_u) > 0 and sum(c[5] for c in counts_u) > 0
    return reads, seqs, peak, want


@pytest.mark.parametrize("k", FUZZ_KS)
def test_fuzz_against_dicts(KT, k):
    import torch
    reads, seqs, peak, want = fuzz_expected(k)
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, seqs)
    if k >= 45:
        assert is_wide(r) and is_wide(a)
    if k <= 32:
        assert not is_wide(r) and not is_wide(a)
    for thre, (want_counts, want_runs) in want.items():
        rep = r.copy_report(a, seqs, thre, peak)
        print(k, thre, peak, summary(want_counts, want_runs), summary(rep.counts, rep.run_tuples()))
        check(rep, want_counts, want_runs, (k, thre))
    # host text and device text give the same object
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert r.copy_report_device(a, d, offs, 3, peak) == r.copy_report(a, seqs, 3, peak)
    r.close()
    a.close()


def small_workload(seed, k, G=20_000, cov=8):
    """reads of a genome and sequences that hold pieces of it 1, 2 and 4 times, with lower case and separators"""
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, G)
    reads = synth.make_reads_stream(rng, genome, cov, 150, 0.003).tobytes()
    g = genome.tobytes()
    asm = synth.make_assembly(rng, genome, err=2e-3, n_every=7000, n_len=30).tobytes()
    seqs = [asm, g[2000:6500] + b"N" + g[2000:6500].lower() + b"N" + revcomp(g[2000:6500]), b"", g[:k - 1], g[9000:9000 + TILE + k]]
    return reads, seqs


def test_an_assembly_table_not_counted_from_the_scanned_text(KT):
    """windows the assembly's table does not have: a == 0, so e >= 1 is `excess` whatever e is, and sum_asm stays 0 there"""
    k = 31
    reads, seqs = small_workload(5, k)
    other = [seqs[0][:8000]]                                   # A holds the first 8000 bases of the first sequence only
    rd, ad = kmer_dict([reads], k), kmer_dict(other, k)
    peak = peak_rule(histo_of(rd), 2)
    want_counts, want_runs = expected(seqs, k, rd, ad, 2, peak)
    cr, ca = dict_counter(rd), dict_counter(ad)
    pairs = [(c, a) for s in seqs for c, a in zip(window_counts(s, k, cr), window_counts(s, k, ca)) if c is not None]
    n_absent_excess = sum(1 for c, a in pairs if a == 0 and c >= 2 and (2 * c + peak) // (2 * peak) >= 1)
    assert n_absent_excess > 5000 and want_counts[2] == want_counts[3] == (0, 0, 0, 0, 0, 0)
    assert sum(c[2] for c in want_counts) >= n_absent_excess
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, other)
    check(r.copy_report(a, seqs, 2, peak), want_counts, want_runs, "foreign A")
    r.close()
    a.close()


@pytest.mark.parametrize("r_slots,a_slots,r_wide,a_wide", [(1 << 22, 1 << 16, False, True), (1 << 16, 1 << 22, True, False)])
def test_narrow_against_wide(KT, r_slots, a_slots, r_wide, a_wide):
    """k = 37 is wide below 2^21 slots and narrow from there on: a small workload in tables of two sizes"""
    k = 37
    reads, seqs = small_workload(77, k)
    rd, ad = kmer_dict([reads], k), kmer_dict(seqs, k)
    peak = peak_rule(histo_of(rd), 2)
    r = KT(k, min_slots=r_slots)
    r.count_bases(reads)
    a = asm_table(KT, k, seqs, a_slots)
    assert (is_wide(r), is_wide(a)) == (r_wide, a_wide)
    for thre in (0, 2):
        want_counts, want_runs = expected(seqs, k, rd, ad, thre, peak)
        assert {x[3] for x in want_runs} == {EXCESS, DEFICIT}
        check(r.copy_report(a, seqs, thre, peak), want_counts, want_runs, (r_slots, a_slots, thre))
    r.close()
    a.close()


def test_scan_through_owner_shards_equals_whole_table(KT):
    from test_gpu_shard import make_shards, workload
    k = 37
    genome, reads, asm = workload(321, 200_000, k)
    full = KT(k, min_slots=1 << 21)
    full.count_bases(reads)
    shards, _ = make_shards(KT, full, 2, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    seqs = [asm, asm[1000:90_000].lower(), asm[:36], "", asm[5000:9000], "ACGT" * 500]
    a = asm_table(KT, k, seqs)
    peak = peak_rule(full.histogram(), 3)
    for thre in (0, 3):
        want = full.copy_report(a, seqs, thre, peak)
        kinds = {x[3] for x in want.run_tuples()}
        assert kinds == {EXCESS, DEFICIT} and len(want.runs) >= 10
        assert shards[0].copy_report(a, seqs, thre, peak) == want
        assert shards[1].copy_report(a, seqs, thre, peak) == want
    with pytest.raises(Exception, match="whole table"):
        full.copy_report(shards[0], seqs, 3, peak)            # an attached table as the assembly
    for t in shards + [full, a]:
        t.close()


def test_more_runs_than_the_first_buffer_holds(KT):
    """every other window `deficit`: R holds the k-mers at the even positions of a random sequence only, A all of them, thre = 0 --
    a window R lacks has c == 0, e == 0 < a.  150 000 runs of one window each are more than the scan's first list of partial runs
    has room for (windows / 64 + 65 536)"""
    k = 21
    rng = np.random.default_rng(77)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300_000)].tobytes()
    reads = b"N".join(s[i:i + k] for i in range(0, len(s) - k + 1, 2))
    rd, ad = kmer_dict([reads], k), kmer_dict([s], k)
    want_counts, want_runs = expected([s], k, rd, ad, 0, 1)
    assert len(want_runs) > 300_000 // 64 + 65_536 and all(r[2] == 1 and r[3] == DEFICIT for r in want_runs[:1000])
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, [s])
    rep = r.copy_report(a, [s], 0, 1)
    check(rep, want_counts, want_runs, "alternating")
    assert rep.retried
    # a peak beyond every count: e == 0 everywhere, every window is deficit -- one run (or a few, where a k-mer occurs twice)
    rep = r.copy_report(a, [s], 0, 1000)
    check(rep, *expected([s], k, rd, ad, 0, 1000), "one run")
    assert len(rep.runs) == 1 and rep.run_tuples()[0][:4] == (0, 0, len(s) - k + 1, DEFICIT) and not rep.retried
    r.close()
    a.close()


def test_ten_calls_give_identical_results_and_leave_the_tables_alone(KT):
    k = 31
    reads, seqs = small_workload(9, k, G=100_000, cov=10)
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, seqs)

    def entries(t):
        e = t.export_entries()
        return e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))].tobytes()
    before = entries(r), entries(a), r.info(), a.info()
    peak = peak_rule(r.histogram(), 2)
    first = r.copy_report(a, seqs, 2, peak)
    assert len(first.runs) > 100
    krep = r.kmer_report(seqs, 2)
    for _ in range(9):
        assert r.copy_report(a, seqs, 2, peak) == first
    assert r.kmer_report(seqs, 2) == krep                      # a report and a copy scan of one table keep their own buffers
    assert (entries(r), entries(a), r.info(), a.info()) == before
    r.close()
    a.close()


def test_bad_arguments_are_errors(KT):
    from jasper_amd import _lib
    r = KT(31, min_slots=1 << 16)
    r.count_bases(b"ACGT" * 100)
    a = KT(31, min_slots=1 << 16)
    a.count_bases(b"ACGT" * 100)
    other = KT(33, min_slots=1 << 16)
    other.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    with pytest.raises(_lib.JasperHipError, match="same table"):
        r.copy_report(r, seqs, 1, 10)
    with pytest.raises(_lib.JasperHipError, match="different k"):
        r.copy_report(other, seqs, 1, 10)
    with pytest.raises(_lib.JasperHipError, match="peak"):
        r.copy_report(a, seqs, 1, 0)
    with pytest.raises(_lib.JasperHipError, match="peak"):
        r.copy_report(a, [], 1, 0)                            # (also with nothing to scan)
    with pytest.raises(TypeError):
        r.copy_report(None, seqs, 1, 10)
    assert r.copy_report(a, seqs, 1, 10).counts[0][:2] == (170, 170)
    for t in (r, a, other):
        t.close()


def test_empty_tables(KT):
    k = 31
    reads, seqs = small_workload(10, k)
    rd, ad = kmer_dict([reads], k), kmer_dict(seqs, k)
    peak = peak_rule(histo_of(rd), 2)
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, seqs)
    empty = KT(k, min_slots=1 << 16)                  # never counted into: logically empty, its memory was never written
    check(r.copy_report(empty, seqs, 2, peak), *expected(seqs, k, rd, {}, 2, peak), "empty A")
    empty.count_bases(b"ACGTTGCATTGACCA" * 30)
    empty.clear()                                     # cleared: logically empty again
    rep = r.copy_report(empty, seqs, 2, peak)
    check(rep, *expected(seqs, k, rd, {}, 2, peak), "cleared A")
    assert all(c[3] == 0 and c[5] == 0 for c in rep.counts) and sum(c[2] for c in rep.counts) > 10_000
    r.clear()                                         # an empty R: at thre 0 every window the assembly has is deficit
    rep = r.copy_report(a, seqs, 0, peak)
    check(rep, *expected(seqs, k, {}, ad, 0, peak), "empty R")
    assert all(c[2] == 0 and c[4] == 0 and c[3] == c[1] for c in rep.counts)
    assert r.copy_report(a, seqs, 1, peak).run_tuples() == []
    assert r.copy_report(a, [], 1, peak).counts == [] and r.copy_report(a, ["", "ACG"], 1, peak).counts == [(0,) * 6] * 2
    for t in (r, a, empty):
        t.close()
