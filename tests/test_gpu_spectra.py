"""GPU: the copy-number k-mer spectrum (KmerTable.spectrum, jasper_table_spectrum) against a restatement of its semantics fed by
independent counts: the dict of a golden case's dump.txt.gz (printed by the real `jellyfish dump -c`) or a Python dict of the
reads' canonical k-mers, joined in Python with a dict of the assembly's canonical k-mers.  Nothing expected here comes from the
code under test.

Semantics (include/jasper_hip.h): S[m][c], m = min(count in the assembly table, 5), c = min(min(count in the read table,
2^32-1), 10001); for c >= 1 the distinct keys of the reads, S[m][0] for m >= 1 the distinct keys only the assembly has."""
import re

import numpy as np
import pytest

from golden_util import Case, case_names

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
ROWS, COLS = 6, 10002
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def kmer_dict(seqs, k):
    """canonical k-mer (bytes) -> occurrences over the sequences: upper-cased, every maximal stretch of >= k ACGT bytes walked"""
    d = {}
    for s in seqs:
        b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
        for m in re.finditer(rb"[ACGT]{%d,}" % k, b.upper()):
            t = m.group()
            for i in range(len(t) - k + 1):
                km = t[i:i + k]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                d[key] = d.get(key, 0) + 1
    return d


def restate(rd, ad):
    """the matrix from the reads' dict and the assembly's dict"""
    S = np.zeros((ROWS, COLS), dtype=np.uint64)
    for key, c in rd.items():
        if c > 0:
            S[min(ad.get(key, 0), 5)][min(min(c, U32), 10001)] += 1
    for key, m in ad.items():
        if m > 0 and rd.get(key, 0) == 0:
            S[min(m, 5)][0] += 1
    return S


def histo_of(d):
    h = [0] * COLS
    for c in d.values():
        if c > 0:
            h[min(c, 10001)] += 1
    return h


def numbers(S, t):
    """(solid, found, asm_distinct, asm_only, row sums over the columns >= 1)"""
    S = np.asarray(S)
    return (int(S[:, t:].sum()), int(S[1:, t:].sum()), int(S[1:, :].sum()), int(S[1:, 0].sum()), [int(S[m, 1:].sum()) for m in range(ROWS)])


def check_invariants(S, r_histo, a_histo):
    """sum over m of S[m][c] = R's histogram for c >= 1; sum over c of S[m][c] = A's histogram, bins 5.. summed into row 5"""
    S = np.asarray(S)
    assert int(S[0, 0]) == 0
    assert [int(v) for v in S[:, 1:].sum(axis=0)] == list(r_histo[1:])
    assert [int(v) for v in S[1:, :].sum(axis=1)] == list(a_histo[1:5]) + [sum(a_histo[5:])]


def asm_table(KT, k, seqs, min_slots=1 << 16):
    """the sequences counted into a table of their own, joined by a separator byte"""
    a = KT(k, min_slots=min_slots)
    a.count_bases(b"N".join(s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs))
    return a


def is_wide(t):
    """the low 64 remainder bits of a slot's key are in a second array when 2k - log2(slots) > 53 (csrc/kmer.hpp: wide_rem)"""
    return 2 * t.k - (t.info()["slots"].bit_length() - 1) > 53


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


# (solid, found, asm_distinct, asm_only, row sums 0..5 over columns >= 1), computed on the CPU from the committed dumps
ANCHORS = {"cluster_k25": (5957, 5526, 5976, 396, [9545, 5580, 0, 0, 0, 0]),
           "edges_k19": (2965, 2689, 2857, 160, [4093, 2650, 47, 0, 0, 0]),
           "rolling_k25": (11400, 4536, 4648, 78, [44769, 3943, 627, 0, 0, 0]),
           "simple_k63": (3925, 3362, 3937, 566, [7452, 3371, 0, 0, 0, 0])}


def test_anchored_cases_exist():
    assert set(ANCHORS) <= set(case_names()) and len(case_names()) == 17


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    rd = {key.encode(): v for key, v in c.dump().items()}
    ad = kmer_dict(seqs, c.k)
    want = restate(rd, ad)
    if name == "rolling_k25":
        assert max(rd.values()) == 879
    r = KT(c.k, min_slots=1 << 16)
    r.count_text(c.reads_text())
    a = asm_table(KT, c.k, seqs)
    spec = r.spectrum(a)
    r_histo, a_histo = r.histogram(), a.histogram()
    r.close()
    a.close()
    print(name, numbers(spec.cells, c.thre), numbers(want, c.thre))
    assert spec.cells.shape == (ROWS, COLS) and spec.cells.dtype == np.uint64
    assert (spec.cells == want).all(), name
    assert numbers(spec.cells, c.thre) == numbers(want, c.thre)
    if name in ANCHORS:
        assert numbers(want, c.thre) == ANCHORS[name]
        assert numbers(spec.cells, c.thre) == ANCHORS[name]
    check_invariants(spec.cells, r_histo, a_histo)
    check_invariants(want, histo_of(rd), histo_of(ad))
    assert r_histo == histo_of(rd) and a_histo == histo_of(ad)
    assert spec.seconds > 0


def revcomp(b):
    return bytes(b).upper().translate(_COMP)[::-1]


def fuzz_workload(seed, k, G=60_000, cov=30):
    """reads (with two homopolymer reads whose k-mers pass the LDS columns and column 10001) and an assembly's sequences that fill
    every row: segments present 2, 3, 4, 5 and 7 times in all (once as the reverse complement), lower case, N stretches, stray
    bytes, an empty sequence, sequences shorter than k"""
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, G)
    reads = synth.make_reads_stream(rng, genome, cov, 150, 0.003).tobytes()
    reads += b"N" + b"A" * 20_000 + b"N" + b"C" * (3000 + k - 1) + b"N"      # A^k: 20001 - k times (column 10001); C^k: 3000 times
    asm = synth.make_assembly(rng, genome, err=2e-3, n_every=9000, n_len=40).copy()
    n = len(asm)
    a0 = int(rng.integers(0, n - 3000))
    asm[a0:a0 + 2000] = np.frombuffer(asm[a0:a0 + 2000].tobytes().lower(), dtype=np.uint8)
    for p, ch in zip(rng.integers(0, n, 12).tolist(), b"nRY-*.\n\0\xffxU "):
        asm[p] = ch
    g = genome.tobytes()
    seqs = [asm.tobytes(), b"", g[100:100 + k - 1], g[200:200 + k].lower()]
    if k > 1:
        seqs.append(g[:k - 1] + b"N" + g[k:2 * k - 1])                       # no k-mer at all
    L = 400 + k
    for extra, at in ((1, 11_000), (2, 13_000), (3, 15_000), (4, 17_000), (6, 19_000)):      # with the copy in `asm`: 2, 3, 4, 5, 7
        seg = g[at:at + L]
        copies = [seg] * (extra - 1) + [revcomp(seg)]
        seqs.append(b"NN".join(copies))
    seqs.append(b"C" * (k + 2))                                              # C^k three times: row 3 in a column beyond the LDS bins
    seqs.append(synth.ACGT[rng.integers(0, 4, 3000)].tobytes())              # not in the reads (k >= 17)
    return reads, seqs


def check_every_branch(want, k):
    """rows 2, 3, 4, 5 and columns 0, > 2047 and 10001 are non-zero in the expected matrix.  k = 1 has two canonical keys (A, C), both
    in the reads and in the assembly thousands of times, so only row 5 and column 10001 can be filled there."""
    if k == 1:
        assert int(want.sum()) == 2 and int(want[5, 10001]) == 2
        return
    for m in (2, 3, 4, 5):
        assert want[m, 1:].sum() > 0, m
    assert want[:, 0].sum() > 0 and want[:, 2048:].sum() > 0 and want[:, 10001].sum() > 0
    assert want[:, 2048:10001].sum() > 0 and want[1:, 1024:].sum() > 0      # the tail beyond the LDS bins, in a row other than 0 too


def run_pair(KT, k, reads, seqs, r_slots, a_slots):
    rd = kmer_dict([reads], k)
    ad = kmer_dict(seqs, k)
    want = restate(rd, ad)
    r = KT(k, min_slots=r_slots)
    r.count_bases(reads)
    a = asm_table(KT, k, seqs, a_slots)
    spec = r.spectrum(a)
    print(k, r_slots, a_slots, is_wide(r), is_wide(a), numbers(spec.cells, 2), numbers(want, 2))
    assert (spec.cells == want).all()
    check_invariants(spec.cells, r.histogram(), a.histogram())
    return r, a, want


@pytest.mark.parametrize("k", [1, 17, 31, 32, 33, 37, 45, 63, 64])
def test_fuzz_against_dicts(KT, k):
    reads, seqs = fuzz_workload(5200 + k, k)
    assert sum(len(s) for s in seqs) <= 300_000
    r, a, want = run_pair(KT, k, reads, seqs, 1 << 16, 1 << 16)
    check_every_branch(want, k)
    if k >= 45:
        assert is_wide(r) and is_wide(a)
    if k <= 32:
        assert not is_wide(r) and not is_wide(a)
    r.close()
    a.close()


@pytest.mark.parametrize("r_slots,a_slots,r_wide,a_wide", [(1 << 22, 1 << 16, False, True), (1 << 16, 1 << 22, True, False)])
def test_narrow_against_wide(KT, r_slots, a_slots, r_wide, a_wide):
    """k = 37 is wide below 2^21 slots and narrow from there on: a small workload in tables of two sizes"""
    k = 37
    reads, seqs = fuzz_workload(77, k, G=20_000, cov=8)
    r, a, want = run_pair(KT, k, reads, seqs, r_slots, a_slots)
    assert (is_wide(r), is_wide(a)) == (r_wide, a_wide)
    check_every_branch(want, k)
    r.close()
    a.close()


def test_spectrum_through_owner_shards_equals_whole_table(KT):
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
    want = full.spectrum(a)
    assert (want.cells == restate(kmer_dict([reads], k), kmer_dict(seqs, k))).all()
    assert want.cells[2:, 1:].sum() > 0 and want.cells[1:, 0].sum() > 0
    assert shards[0].spectrum(a) == want
    assert shards[1].spectrum(a) == want
    with pytest.raises(Exception, match="whole table"):
        full.spectrum(shards[0])                      # an attached table as the assembly
    for t in shards + [full, a]:
        t.close()


def small_pair(KT, k=31, seed=9):
    reads, seqs = fuzz_workload(seed, k, G=150_000, cov=15)
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    return r, asm_table(KT, k, seqs), reads, seqs


def test_ten_calls_give_identical_cells_and_leave_the_tables_alone(KT):
    r, a, reads, seqs = small_pair(KT)

    def entries(t):
        e = t.export_entries()
        return e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))].tobytes()
    before = entries(r), entries(a), r.info(), a.info()
    first = r.spectrum(a)
    assert (first.cells == restate(kmer_dict([reads], 31), kmer_dict(seqs, 31))).all()
    for _ in range(9):
        assert r.spectrum(a) == first
    assert (entries(r), entries(a), r.info(), a.info()) == before
    r.close()
    a.close()


def test_bad_pairs_are_errors(KT):
    from jasper_amd import _lib
    r = KT(31, min_slots=1 << 16)
    r.count_bases(b"ACGT" * 100)
    other = KT(33, min_slots=1 << 16)
    other.count_bases(b"ACGT" * 100)
    with pytest.raises(_lib.JasperHipError, match="same table"):
        r.spectrum(r)
    with pytest.raises(Exception, match="different k"):
        r.spectrum(other)
    with pytest.raises(TypeError):
        r.spectrum(None)
    r.close()
    other.close()


def test_empty_tables(KT):
    k = 31
    r, a, reads, seqs = small_pair(KT, k, seed=10)
    r_histo, a_histo = r.histogram(), a.histogram()
    empty = KT(k, min_slots=1 << 16)                  # never counted into: logically empty, its memory was never written
    s = r.spectrum(empty)
    assert [int(v) for v in s.cells[0]] == [0] + r_histo[1:] and int(s.cells[1:].sum()) == 0
    empty.count_bases(b"ACGTTGCATTGACCA" * 30)
    empty.clear()                                     # cleared: logically empty again
    s = r.spectrum(empty)
    assert [int(v) for v in s.cells[0]] == [0] + r_histo[1:] and int(s.cells[1:].sum()) == 0
    r.clear()                                         # an empty R: everything the assembly has is assembly-only
    s = r.spectrum(a)
    assert int(s.cells[:, 1:].sum()) == 0 and int(s.cells[0, 0]) == 0
    assert [int(v) for v in s.cells[1:, 0]] == a_histo[1:5] + [sum(a_histo[5:])]
    assert sum(a_histo[2:]) > 0
    for t in (r, a, empty):
        t.close()
