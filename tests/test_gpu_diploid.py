"""GPU: the pair spectrum (KmerTable.spectrum_pair, jasper_table_spectrum_pair) and the pair scan (KmerTable.pair_scan,
jasper_pair_scan) of a diploid assembly against restatements of their semantics fed by Python dicts of canonical k-mer strings: the
dict of a golden case's dump.txt.gz (printed by the real `jellyfish dump -c`) or a dict of the reads' canonical k-mers for R, dicts of
the two haplotypes' for A1 and A2.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h).  P[j][c]: j = (key in A1 ? 1 : 0) | (key in A2 ? 2 : 0), c = min(min(count in R, 2^32-1), 10001);
for c >= 1 the distinct keys of R, column 0 the distinct keys of A1 u A2 that R does not hold.  Scan of one haplotype's sequences against
R and the OTHER haplotype's table O: window i is valid iff all k bytes are ACGTacgt; c = its canonical k-mer's count in R clamped to
2^32-1, b = its count in O; unreliable iff c < thre, absent iff c == 0; private_solid (1) iff b == 0 and c >= thre, private_weak (2)
iff b == 0 and c < thre; per sequence (windows, valid, unreliable, absent, private_solid, private_weak); a run is a maximal range of
consecutive windows of one non-zero class: (seq, start, n_kmers, kind, sum_reads)."""
import random

import numpy as np
import pytest

import layout_util as lu
from golden_util import Case, case_names
from test_gpu_copies import asm_table, dict_counter, histo_of, is_wide, kmer_dict, window_counts

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
ROWS, COLS = 4, 10002
TILE = 4096
SOLID, WEAK = 1, 2


def restate_pair(rd, d1, d2):
    """the matrix from the reads' dict and the two haplotypes' dicts"""
    P = np.zeros((ROWS, COLS), dtype=np.uint64)
    for key, c in rd.items():
        if c > 0:
            P[(1 if d1.get(key, 0) > 0 else 0) | (2 if d2.get(key, 0) > 0 else 0)][min(min(c, U32), 10001)] += 1
    for key in set(d1) | set(d2):
        j = (1 if d1.get(key, 0) > 0 else 0) | (2 if d2.get(key, 0) > 0 else 0)
        if j and rd.get(key, 0) == 0:
            P[j][0] += 1
    return P


def spectrum_rows(rd, ad):
    """sum over m >= 1 of the copy-number spectrum S[m][c] of (R, A), from the dicts: the keys A holds, by their column"""
    v = np.zeros(COLS, dtype=np.uint64)
    for key, m in ad.items():
        if m > 0:
            v[min(min(rd.get(key, 0), U32), 10001)] += 1
    return v


def check_identities(P, s1_rows, s2_rows, r_histo):
    """the three identities of the issue: rows 1 + 3 = S1's rows m >= 1, rows 2 + 3 = S2's, and the columns >= 1 add up to R's histogram"""
    P = np.asarray(P)
    assert int(P[0, 0]) == 0
    assert (P[1] + P[3] == np.asarray(s1_rows, dtype=np.uint64)).all()
    assert (P[2] + P[3] == np.asarray(s2_rows, dtype=np.uint64)).all()
    assert [int(v) for v in P[:, 1:].sum(axis=0)] == list(r_histo[1:])


def restate_scan(seqs, k, rd, od, thre):
    """(counts, runs) of the scan's semantics from the reads' dict and the OTHER haplotype's dict"""
    cr, co = dict_counter(rd), dict_counter(od)
    counts, runs = [], []
    for si, s in enumerate(seqs):
        wc, wo = window_counts(s, k, cr), window_counts(s, k, co)
        valid = un = ab = ps = pw = 0
        cur = None
        for i, (c, b) in enumerate(zip(wc, wo)):
            cls = 0
            if c is not None:
                valid += 1
                un += c < thre
                ab += c == 0
                if b == 0:
                    cls = SOLID if c >= thre else WEAK
                ps += cls == SOLID
                pw += cls == WEAK
            if cur is not None and cur[3] != cls:
                runs.append(tuple(cur))
                cur = None
            if cls:
                if cur is None:
                    cur = [si, i, 0, cls, 0]
                cur[2] += 1
                cur[4] += c
        if cur is not None:
            runs.append(tuple(cur))
        counts.append((len(wc), valid, un, ab, ps, pw))
    return counts, runs


def scan_summary(counts, runs):
    """(valid, unreliable, absent, private_solid, private_weak, runs)"""
    return tuple(sum(c[i] for c in counts) for i in range(1, 6)) + (len(runs),)


def check_scan(rep, want_counts, want_runs, what):
    assert rep.counts == want_counts, what
    got = rep.run_tuples()
    assert len(got) == len(want_runs), (what, len(got), len(want_runs))
    assert got == want_runs, what


def fasta_records(text):
    seqs = []
    for ln in text.splitlines():
        if ln.startswith(">"):
            seqs.append([])
        elif seqs:
            seqs[-1].append(ln.strip())
    return ["".join(s) for s in seqs]


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


# threshold, P's row sums, solid, found (asm, alt, both), scan of asm against alt and of alt against asm as (valid, unreliable, absent,
# private_solid, private_weak, runs): computed on the CPU from the committed fixtures
ANCHORS = {"cluster_k25": (5, [9114, 431, 431, 5545], 5957, (5526, 5957, 5957), (5976, 450, 396, 0, 431, 12), (5976, 19, 3, 431, 0, 12)),
           "edges_k19": (5, [4003, 110, 90, 2747], 2965, (2689, 2779, 2779), (2904, 168, 160, 0, 110, 6), (2904, 58, 50, 90, 0, 5)),
           "rolling_k25": (5, [44721, 97, 48, 4551], 11400, (4536, 4559, 4584), (5275, 112, 78, 25, 72, 4), (5276, 40, 6, 48, 0, 2)),
           "simple_k63": (3, [6889, 562, 563, 3375], 3925, (3362, 3925, 3925), (3937, 575, 566, 0, 562, 9), (3938, 13, 4, 563, 0, 9))}


def pair_numbers(P, t):
    P = np.asarray(P)
    t = max(1, t)
    return ([int(v) for v in P.sum(axis=1)], int(P[:, t:].sum()),
            (int(P[[1, 3], t:].sum()), int(P[[2, 3], t:].sum()), int(P[1:, t:].sum())))


def test_anchored_cases_exist():
    assert set(ANCHORS) <= set(case_names()) and len(case_names()) == 17


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs1 = c.batch()
    seqs2 = fasta_records(c.fixed_fa())
    assert seqs2 and seqs1 != seqs2
    k, thre = c.k, c.thre
    rd = {key.encode(): v for key, v in c.dump().items()}
    d1, d2 = kmer_dict(seqs1, k), kmer_dict(seqs2, k)
    want = restate_pair(rd, d1, d2)
    check_identities(want, spectrum_rows(rd, d1), spectrum_rows(rd, d2), histo_of(rd))
    want12 = restate_scan(seqs1, k, rd, d2, thre)
    want21 = restate_scan(seqs2, k, rd, d1, thre)
    r = KT(k, min_slots=1 << 16)
    r.count_text(c.reads_text())
    a1, a2 = asm_table(KT, k, seqs1), asm_table(KT, k, seqs2)
    got = r.spectrum_pair(a1, a2)
    s1, s2 = r.spectrum(a1), r.spectrum(a2)
    r_histo = r.histogram()
    scan12, scan21 = r.pair_scan(a2, seqs1, thre), r.pair_scan(a1, seqs2, thre)
    rep1, rep2 = r.kmer_report(seqs1, thre), r.kmer_report(seqs2, thre)
    for t in (r, a1, a2):
        t.close()
    print(name, thre, pair_numbers(want, thre), scan_summary(*want12), scan_summary(*want21))
    print(name, thre, pair_numbers(got.cells, thre), scan_summary(scan12.counts, scan12.run_tuples()), scan_summary(scan21.counts, scan21.run_tuples()))
    assert got.cells.shape == (ROWS, COLS) and got.cells.dtype == np.uint64
    assert (got.cells == want).all(), name
    check_identities(got.cells, s1.cells[1:].sum(axis=0), s2.cells[1:].sum(axis=0), r_histo)
    check_scan(scan12, *want12, (name, "asm against alt"))
    check_scan(scan21, *want21, (name, "alt against asm"))
    assert [x[:4] for x in scan12.counts] == [tuple(x) for x in rep1.counts]
    assert [x[:4] for x in scan21.counts] == [tuple(x) for x in rep2.counts]
    assert int(want[1].sum()) > 0 and int(want[2].sum()) > 0, "vacuous case: no private k-mers on one side"
    if name in ANCHORS:
        at, rows, solid, found, sc12, sc21 = ANCHORS[name]
        assert at == thre
        assert pair_numbers(want, thre) == (rows, solid, found)
        assert (scan_summary(*want12), scan_summary(*want21)) == (sc12, sc21)
    assert got.seconds > 0 and scan12.seconds > 0 and not scan12.retried


# ---- the join at its limits ----------------------------------------------------------------------------------------------------------
BIG = [1023, 1024, 10000, 10001, 12000, 2**32, 2**32 + 5, 2**40]


def put(table, d, hashes, kmers, counts):
    """import the keys into the table and add them to its dict"""
    table.import_entries(lu.entries(hashes, counts))
    for km, c in zip(kmers, counts):
        d[km.encode()] = d.get(km.encode(), 0) + c


def test_join_full_probe_chains(KT):
    """k = 37, A1 at 2^16 and A2 at 2^17 slots (wide), R at 2^22 (narrow): 1024 keys of ONE home fill all probe offsets of that home in A2,
    and 1024 of the last home in A1 (the chain wraps round the table's end).  R probes them with keys the chain holds -- its first, its
    last, every 37th -- and with keys that only share the chain's home (and, the tables being wide, one of the two remainder words), which
    walk the whole chain and find nothing.  A few keys of each chain are in the other table too (they share a home there: a short chain)."""
    k, s1, s2 = 37, 16, 17
    rng = random.Random(3702)
    r, a1, a2 = KT(k, min_slots=1 << 22), KT(k, min_slots=1 << s1), KT(k, min_slots=1 << s2)
    assert not is_wide(r) and is_wide(a1) and is_wide(a2)
    rd, d1, d2 = {}, {}, {}
    taken = set()
    for table, d, s, home, o_table, o_d in ((a2, d2, s2, (1 << s2) // 3, a1, d1), (a1, d1, s1, (1 << s1) - 1, a2, d2)):
        ch, ckm = lu.craft(k, s, home, lu.MAXPROBE, rng)
        put(table, d, ch, ckm, [1 + i % 3 for i in range(lu.MAXPROBE)])
        put(o_table, o_d, ch[520:540], ckm[520:540], [2] * 20)
        taken |= set(ckm)
        near = lu.absent_neighbours(k, s, ch[:4] + ch[-4:], taken, rng)
        assert len(near) >= 8
        taken |= set(near)
        present = sorted(set(range(0, lu.MAXPROBE, 37)) | {lu.MAXPROBE - 1} | set(range(525, 530)))
        put(r, rd, [ch[i] for i in present], [ckm[i] for i in present], [7] * len(present))
        put(r, rd, [lu.hash_of_kmer(km) for km in near], near, [9] * len(near))      # in R, sharing the chain's home, in neither assembly table
    assert a1.info()["slots"] == 1 << s1 and a2.info()["slots"] == 1 << s2, "1024 keys of one home fit its probe sequence: no growth"
    want = restate_pair(rd, d1, d2)
    assert want[0, 9] >= 16 and want[1, 7] >= 20 and want[2, 7] >= 20 and want[3, 7] == 10 and want[3, 0] == 30 and want[1, 0] > 900 and want[2, 0] > 900
    got = r.spectrum_pair(a1, a2)
    assert (got.cells == want).all()
    assert (r.spectrum_pair(a2, a1).cells[[0, 2, 1, 3]] == want).all()
    for t in (r, a1, a2):
        t.close()


def test_join_narrow_reads_wide_assemblies_and_big_counts(KT):
    """k = 37: R at 2^22 slots is narrow (and its sweep makes two trips under the cap of 2048 workgroups of 256 threads x 4 slots), A1 at
    2^16 and A2 at 2^17 are wide.  Counts around the LDS columns' end, the last column and 2^32 in every row."""
    k = 37
    rng = random.Random(3701)
    nrng = np.random.default_rng(3701)
    from jasper_amd import synth
    genome = synth.make_genome(nrng, 20_000)
    reads = synth.make_reads_stream(nrng, genome, 8, 150, 0.003).tobytes()
    reads += b"N" + b"A" * (12000 + k - 1) + b"N" + b"C" * (10001 + k - 1) + b"N"      # a run of one base: A^k 12000 times, C^k 10001 times
    g = genome.tobytes()
    text1 = [g[:12_000], b"A" * (k + 1), synth.ACGT[nrng.integers(0, 4, 2000)].tobytes()]            # A^k in A1 only; C^k in neither
    text2 = [g[8000:], synth.ACGT[nrng.integers(0, 4, 2000)].tobytes()]
    r = KT(k, min_slots=1 << 22)
    a1 = KT(k, min_slots=1 << 16)
    a2 = KT(k, min_slots=1 << 17)
    r.count_bases(reads)
    a1.count_bases(b"N".join(text1))
    a2.count_bases(b"N".join(text2))
    rd, d1, d2 = kmer_dict([reads], k), kmer_dict(text1, k), kmer_dict(text2, k)
    s_r, s1, s2 = lu.log2_slots(r), lu.log2_slots(a1), lu.log2_slots(a2)
    assert (s_r, s1, s2) == (22, 16, 17) and not is_wide(r) and is_wide(a1) and is_wide(a2)
    assert (1 << s_r) > 2048 * 256 * 4, "R's sweep makes more than one trip"

    # the big counts in every row: 4 x len(BIG) random keys
    hs, kms = lu.craft(k, 0, 0, 4 * len(BIG), rng)
    for row in range(4):
        sl = slice(row * len(BIG), (row + 1) * len(BIG))
        put(r, rd, hs[sl], kms[sl], BIG)
        if row & 1:
            put(a1, d1, hs[sl], kms[sl], [1 + i % 3 for i in range(len(BIG))])
        if row & 2:
            put(a2, d2, hs[sl], kms[sl], [2] * len(BIG))
    assert a1.info()["slots"] == 1 << s1 and a2.info()["slots"] == 1 << s2 and r.info()["slots"] == 1 << s_r, "no table grew"
    want = restate_pair(rd, d1, d2)
    for row in range(4):
        for c in (1023, 1024, 10000):
            assert want[row, c] >= 1, (row, c)
        assert want[row, 10001] >= 5, row                      # 10001, 12000 and the three counts of 2^32 and more
    assert want[1, 0] > 0 and want[2, 0] > 0 and want[3, 1:].sum() > 1000
    shared_before = int(want[3, 0])                            # (where the reads' coverage left a hole in the stretch both texts hold)
    got = r.spectrum_pair(a1, a2)
    print(pair_numbers(got.cells, 2), pair_numbers(want, 2))
    assert (got.cells == want).all()
    check_identities(got.cells, r.spectrum(a1).cells[1:].sum(axis=0), r.spectrum(a2).cells[1:].sum(axis=0), r.histogram())
    assert r.spectrum_pair(a1, a2) == got                      # two calls give equal results
    swapped = r.spectrum_pair(a2, a1)                          # the haplotypes swapped: rows 1 and 2 change places
    assert (swapped.cells[[0, 2, 1, 3]] == got.cells).all()
    # a key of A1 u A2 that R does not hold and both haplotypes do: counted once, by A1's sweep
    shared = lu.craft(k, 0, 0, 3, rng)
    put(a1, d1, *shared, [1, 2, 3])
    put(a2, d2, *shared, [4, 4, 4])
    want = restate_pair(rd, d1, d2)
    assert want[3, 0] == shared_before + 3
    assert (r.spectrum_pair(a1, a2).cells == want).all()
    assert (r.spectrum_pair(a2, a1).cells[[0, 2, 1, 3]] == want).all()
    for t in (r, a1, a2):
        t.close()


def test_join_with_empty_tables(KT):
    k = 31
    from jasper_amd import synth
    nrng = np.random.default_rng(31)
    genome = synth.make_genome(nrng, 30_000)
    reads = synth.make_reads_stream(nrng, genome, 8, 150, 0.003).tobytes()
    g = genome.tobytes()
    text = g[:20_000] + b"N" + synth.ACGT[nrng.integers(0, 4, 1000)].tobytes()
    rd, ad = kmer_dict([reads], k), kmer_dict([text], k)
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    a = asm_table(KT, k, [text])
    fresh = KT(k, min_slots=1 << 16)                  # never counted into: logically empty, its memory was never written
    nokmer = KT(k, min_slots=1 << 16)
    nokmer.count_bases(g[:k - 1] + b"N" + g[100:100 + k - 1])      # counted, but the text holds no k-mer
    assert nokmer.info()["distinct"] == 0
    for empty in (fresh, nokmer):
        want = restate_pair(rd, ad, {})
        assert want[1].sum() > 0 and want[1, 0] > 0 and want[2].sum() == 0 and want[3].sum() == 0
        assert (r.spectrum_pair(a, empty).cells == want).all()
        assert (r.spectrum_pair(empty, a).cells == restate_pair(rd, {}, ad)).all()
    assert (r.spectrum_pair(fresh, nokmer).cells == restate_pair(rd, {}, {})).all()
    r.clear()                                         # an empty R: everything the haplotypes hold is in column 0
    got = r.spectrum_pair(a, fresh).cells
    assert (got == restate_pair({}, ad, {})).all() and int(got[:, 1:].sum()) == 0 and int(got[1, 0]) == len(ad)
    for t in (r, a, fresh, nokmer):
        t.close()


def test_bad_arguments_are_errors(KT):
    from jasper_amd import _lib
    r, a1, a2 = (KT(31, min_slots=1 << 16) for _ in range(3))
    other = KT(33, min_slots=1 << 16)
    for t in (r, a1, a2, other):
        t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for x, y, z in ((r, r, a2), (r, a1, r), (r, a1, a1)):                      # the same handle twice, in each position
        with pytest.raises(_lib.JasperHipError, match="same table"):
            x.spectrum_pair(y, z)
    for y, z in ((other, a2), (a1, other)):
        with pytest.raises(_lib.JasperHipError, match="different k"):
            r.spectrum_pair(y, z)
    with pytest.raises(_lib.JasperHipError, match="different k"):
        other.spectrum_pair(a1, a2)
    for y, z in ((None, a2), (a1, None)):
        with pytest.raises(TypeError):
            r.spectrum_pair(y, z)
    with pytest.raises(_lib.JasperHipError, match="same table"):
        r.pair_scan(r, seqs, 1)
    with pytest.raises(_lib.JasperHipError, match="different k"):
        r.pair_scan(other, seqs, 1)
    with pytest.raises(TypeError):
        r.pair_scan(None, seqs, 1)
    assert int(r.spectrum_pair(a1, a2).cells[3].sum()) == 2                    # (ACGT repeated: two canonical 31-mers)
    assert r.pair_scan(a1, seqs, 1).counts == [(170, 170, 0, 0, 0, 0)]
    assert r.pair_scan(a1, [], 1).counts == [] and r.pair_scan(a1, ["", "ACG"], 1).counts == [(0,) * 6] * 2
    a2.close()
    with pytest.raises(TypeError):                                             # a closed table, as for spectrum and copy_report
        r.spectrum_pair(a1, a2)
    with pytest.raises(TypeError):
        r.pair_scan(a2, seqs, 1)
    for t in (r, a1, other):
        t.close()


# ---- the scan at its limits ----------------------------------------------------------------------------------------------------------
def other_base(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


def scan_workload(k, seed):
    """(reads text, this haplotype's sequences, the other haplotype's sequences, the planted places).  The truth T is random; the other
    haplotype holds T; this haplotype holds T with SNPs (the reads hold both alleles: solid), wrong bases (the reads hold T's only: weak)
    and one wrong base BOTH haplotypes have (unreliable, not private).  The reads hold every text five times."""
    rng = np.random.default_rng(seed)

    def rand(n):
        return bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes())

    T = rand(4 * TILE + 700 + k - 1)                           # four tiles and a piece: at least 3 * 4096 + k windows
    snps = {"ends_4095": TILE - 1,                             # windows 4096 - k .. 4095: the run ends on a tile's last window
            "starts_8192": 2 * TILE + k - 1,                   # windows 8192 .. 8192 + k - 1: the run starts on a tile's first window
            "crosses": 3 * TILE + 5,                           # windows 12288 + 5 - (k - 1) .. 12288 + 5: across one seam
            "plain": 1000}
    errs = [300, 2000, 2000 + k + 3, 6000, 4 * TILE + 300]     # single wrong bases; two of them k + 3 apart (two runs, three windows between)
    both_wrong = 10_000
    S_solid = bytearray(T)
    for p in snps.values():
        S_solid[p] = other_base(T[p])
    H = bytearray(T)
    H[both_wrong] = other_base(T[both_wrong])
    S = bytearray(S_solid)
    S[both_wrong] = H[both_wrong]
    for p in errs:
        S[p] = other_base(T[p])
    # a stretch of 9000 bases that only this haplotype and the reads hold: a solid run over two seams
    fa, ins, fb = rand(700), rand(9000), rand(600)
    S2, H2 = fa + ins + fb, fa + fb
    # an insertion the reads cover in part only: they hold S3[: TILE + k - 1], so window 4095 is the last solid one and 4096 the first weak one
    ga, gi, gb = rand(4000), rand(300), rand(500)
    S3, H3 = ga + gi + gb, ga + gb
    S3_reads = S3[:TILE + k - 1]
    # N runs and a lower-case stretch, with a SNP inside the lower case and a wrong base next to an N run
    U = rand(3000)
    S4 = bytearray(U)
    S4[1500] = other_base(U[1500])
    S4_solid = bytearray(S4)
    S4[2500] = other_base(U[2500])
    S4m = bytes(S4[:700]) + b"NNNN" + bytes(S4[700:1200]) + bytes(S4[1200:1900]).lower() + b"n" + bytes(S4[1900:])
    seqs = [bytes(S), bytes(S2), bytes(S3), S4m, bytes(T[50:50 + k - 1]), bytes(T[90:90 + k]), b""]
    other = [bytes(H), bytes(H2), bytes(H3), bytes(U)]
    read_texts = [bytes(T), bytes(S_solid), bytes(S2), bytes(H2), bytes(S3_reads), bytes(H3), bytes(U), bytes(S4_solid)]
    return read_texts, seqs, other, dict(snps=snps, errs=errs, both_wrong=both_wrong)


def times(d, n):
    return {key: c * n for key, c in d.items()}


@pytest.mark.parametrize("k", [21, 37])
def test_scan_planted_runs_at_the_tile_seams(KT, k):
    read_texts, seqs, other, at = scan_workload(k, 900 + k)
    COPIES, THRE = 5, 3
    rd = times(kmer_dict(read_texts, k), COPIES)
    od = kmer_dict(other, k)
    want = {t: restate_scan(seqs, k, rd, od, t) for t in (0, 1, THRE, U32)}
    counts, runs = want[THRE]
    runs0 = [x for x in runs if x[0] == 0]
    sn = at["snps"]
    assert (0, TILE - k, k, SOLID, COPIES * k) in runs0, "a run that ends on window 4095"
    assert (0, 2 * TILE, k, SOLID, COPIES * k) in runs0, "a run that starts on window 8192"
    assert (0, sn["crosses"] - k + 1, k, SOLID, COPIES * k) in runs0, "a run across one seam"
    for p in at["errs"]:
        assert (0, p - k + 1, k, WEAK, 0) in runs0, "weak runs from single wrong bases"
    assert counts[0][2] == counts[0][5] + k and counts[0][5] == len(at["errs"]) * k, "k unreliable windows both haplotypes hold"
    big = [x for x in runs if x[0] == 1]
    # (a junction window is not private where the insertion's first or last bases repeat the flank's: the runs may be a few windows shorter)
    assert len(big) == 1 and big[0][3] == SOLID and 9000 <= big[0][2] <= 9000 + k - 1 and big[0][4] == COPIES * big[0][2], "one solid run"
    assert (big[0][1] + big[0][2] - 1) // TILE - big[0][1] // TILE >= 2, "a solid run over two seams"
    r3 = [x for x in runs if x[0] == 2]
    assert len(r3) == 2 and r3[0][3] == SOLID and r3[0][1] + r3[0][2] == TILE and r3[0][2] > k and r3[0][4] == COPIES * r3[0][2], "a solid run up to window 4095 ..."
    assert r3[1][3] == WEAK and r3[1][1] == TILE and r3[1][2] > 150 and r3[1][4] == 0, "... touches a weak run from window 4096 on"
    assert {x[3] for x in runs if x[0] == 3} == {SOLID, WEAK}
    assert counts[4] == (0,) * 6 and counts[5] == (1, 1, 0, 0, 0, 0) and counts[6] == (0,) * 6
    assert all(x[3] == SOLID for x in want[0][1]) and sum(c[2] for c in want[0][0]) == 0, "a threshold of 0: nothing is weak"
    assert all(x[3] == WEAK for x in want[U32][1])
    r = KT(k, min_slots=1 << 16)
    r.count_bases(b"N".join(b"N".join(read_texts) for _ in range(COPIES)))
    o = asm_table(KT, k, other)
    for t, (wc, wr) in want.items():
        rep = r.pair_scan(o, seqs, t)
        print(k, t, scan_summary(wc, wr), scan_summary(rep.counts, rep.run_tuples()), rep.retried)
        check_scan(rep, wc, wr, (k, t))
        assert [x[:4] for x in rep.counts] == [tuple(x) for x in r.kmer_report(seqs, t).counts]
        assert not rep.retried
    assert r.pair_scan(o, seqs, THRE) == r.pair_scan(o, seqs, THRE)
    # this haplotype's table as the other one: nothing is private
    own = asm_table(KT, k, seqs)
    rep = r.pair_scan(own, seqs, THRE)
    assert rep.run_tuples() == [] and [x[:4] for x in rep.counts] == [x[:4] for x in counts] and all(x[4:] == (0, 0) for x in rep.counts)
    # a table never counted into as the other one: every valid window is private
    fresh = KT(k, min_slots=1 << 16)
    check_scan(r.pair_scan(fresh, seqs, THRE), *restate_scan(seqs, k, rd, {}, THRE), "empty other")
    for t in (r, o, own, fresh):
        t.close()


def test_scan_narrow_reads_against_a_wide_other(KT):
    k = 37
    read_texts, seqs, other, _ = scan_workload(k, 77)
    rd, od = kmer_dict(read_texts, k), kmer_dict(other, k)
    for r_slots, o_slots, wide in (((1 << 22), 1 << 16, (False, True)), (1 << 16, 1 << 22, (True, False))):
        r = KT(k, min_slots=r_slots)
        r.count_bases(b"N".join(read_texts))
        o = asm_table(KT, k, other, o_slots)
        assert (is_wide(r), is_wide(o)) == wide
        check_scan(r.pair_scan(o, seqs, 1), *restate_scan(seqs, k, rd, od, 1), wide)
        r.close()
        o.close()


def test_scan_more_runs_than_the_first_buffer_holds(KT):
    """R holds the k-mers at the even positions of a random sequence only and the other haplotype's table none of them: every window is
    private, solid at the even positions and weak at the odd ones -- 300 000 runs of one window each, more than the scan's first list of
    partial runs has room for (windows / 64 + 65 536), so the scan is repeated with exactly the room it counted"""
    k = 21
    rng = np.random.default_rng(78)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300_000)].tobytes()
    reads = b"N".join(s[i:i + k] for i in range(0, len(s) - k + 1, 2))
    rd = kmer_dict([reads], k)
    want_counts, want_runs = restate_scan([s], k, rd, {}, 1)
    assert len(want_runs) > 300_000 // 64 + 65_536 and all(x[2] == 1 for x in want_runs[:1000]) and {x[3] for x in want_runs[:1000]} == {SOLID, WEAK}
    r = KT(k, min_slots=1 << 16)
    r.count_bases(reads)
    o = KT(k, min_slots=1 << 16)
    rep = r.pair_scan(o, [s], 1)
    check_scan(rep, want_counts, want_runs, "alternating")
    assert rep.retried in (False, True)
    assert r.pair_scan(o, [s], 1) == rep
    r.close()
    o.close()
