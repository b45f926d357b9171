"""GPU: the het-cluster half of the indel scan (KmerTable.indel_scan(.., clusters=N) / indel_scan_device, jasper_indel_scan_clusters)
against the restatement of its semantics in test_het_clusters_host.py, fed by Python dicts of canonical k-mer strings.  Nothing expected
here comes from the code under test.  Every workload also states that the rest of the result is that of the scan without clusters."""
import numpy as np
import pytest

from golden_util import Case, case_names
from test_compound_host import restate_compound
from test_gpu_copies import TILE, dict_counter, is_wide, kmer_dict
from test_het_clusters_host import (FRONT, SEARCHED, applied, cap_workload, dense_workload, planted_pairs, restate_clusters, snp_beside_indel,
                                    substitute)
from test_indels_host import ACGT, rand_bases
from test_indels_mixed_host import plant_strings

pytestmark = pytest.mark.gpu


def check(t, seqs, thre, N, want, what, max_len=4, mixed=False):
    """indel_scan(.., clusters=N).clusters against (counts, records) of the restatement"""
    isc = t.indel_scan(seqs, thre, max_len, mixed=mixed, clusters=N)
    hc = isc.clusters
    assert hc is not None and hc.counts == want[0], (what, hc.counts, want[0])
    got = hc.record_tuples()
    assert len(got) == len(want[1]), (what, len(got), len(want[1]))
    assert got == want[1], what
    assert all(bytes(r["pad"]) == bytes(6) for r in hc.records[:100])
    assert 0 <= hc.seconds <= isc.seconds
    return isc


def table_of(KT, k, reads, min_slots=1 << 16):
    t = KT(k, min_slots=min_slots)
    t.count_bases(b"N".join(reads))
    return t


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable, _lib
    assert KmerTable.report_tile_windows() == TILE and _lib.lib().jasper_indel_front() == FRONT
    return KmerTable


# ---- golden cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    want64, want4 = restate_clusters(seqs, c.k, count, c.thre, 64), restate_clusters(seqs, c.k, count, c.thre, 4)
    assert sum(x[0] for x in want64[0]) == SEARCHED.get(name, 0) and want64[1] == []
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    isc = check(t, seqs, c.thre, 64, want64, name)
    check(t, seqs, c.thre, 4, want4, (name, 4))
    t.close()
    assert not isc.clusters.retried and (isc.clusters.lookups > 0) == (isc.variants.candidates > 0)


# ---- planted pairs -----------------------------------------------------------------------------------------------------------------
def long_pairs(k, n=12000, seed=31):
    """planted_pairs of test_het_clusters_host inside haplotypes of n bases: (h1, h2, pairs)"""
    a, b, pairs, _ = planted_pairs(k)
    rng = np.random.default_rng(seed + k)
    tail = rand_bases(rng, n - len(a))
    return a + tail, b + tail, pairs


@pytest.mark.parametrize("k", [21, 31, 64])
def test_planted_pairs(KT, k):
    """pairs of SNPs 1, 2, 3, 7, k-2 and k-1 apart, one record each from either haplotype's view (at k = 64 the table is wide and the
    last pair is R = 64 = N); the pair k apart lists nothing; N = d + 1 lists a pair, N = d does not"""
    h1, h2, pairs = long_pairs(k)
    reads = [h1] * 5 + [h2] * 5
    count = dict_counter(kmer_dict(reads, k))
    t = table_of(KT, k, reads)
    assert is_wide(t) == (k == 64)
    for mine, other in ((h1, h2), (h2, h1)):
        want = restate_clusters([mine], k, count, 3, 64)
        assert [r[1:5] for r in want[1]] == [(p, d + 1, d + 1, other[p:p + d + 1].decode()) for p, d in pairs]
        check(t, [mine], 3, 64, want, k)
    for N in (8, 7, 3, 2, 1):
        want = restate_clusters([h1], k, count, 3, N)
        assert [r[1] for r in want[1]] == [p for p, d in pairs if d + 1 <= N]
        check(t, [h1], 3, N, want, (k, N))
    t.close()


@pytest.mark.parametrize("k", [21, 31, 64])
def test_a_snp_beside_a_length_difference(KT, k):
    longer, shorter, p = snp_beside_indel(k)
    rng = np.random.default_rng(70 + k)
    tail = rand_bases(rng, 12000)
    longer, shorter = longer + tail, shorter + tail
    reads = [longer] * 5 + [shorter] * 5
    count = dict_counter(kmer_dict(reads, k))
    want = restate_clusters([longer, shorter], k, count, 3, 64)
    assert want[0] == [(1, 1, 1, 0)] * 2 and [r[2] - r[3] for r in want[1]] == [2, -2]
    assert applied(longer, want[1][0]) == shorter and applied(shorter, want[1][1]) == longer
    t = table_of(KT, k, reads)
    check(t, [longer, shorter], 3, 64, want, k)
    t.close()


# ---- what bounds R_max -------------------------------------------------------------------------------------------------------------
def test_weak_contig_kmers_leave_the_site_to_the_compound_scan(KT):
    """two haplotypes that differ at p and p + 5, and a contig that is the first one with two errors of its own at p + 2 and p + 3: the
    candidate at p is there, R_max = 0, nothing is searched here, and compound_scan lists the two errors"""
    k = 31
    rng = np.random.default_rng(3131)
    h1 = rand_bases(rng, 12000)
    p = 5000
    h2 = substitute(h1, [p, p + 5])
    contig = substitute(h1, [p + 2, p + 3])
    for x in (p + 2, p + 3):                              # an error: neither haplotype's base
        assert contig[x] != h2[x]
    reads = [h1] * 5 + [h2] * 5
    count = dict_counter(kmer_dict(reads, k))
    st = {}
    want = restate_clusters([contig, h1], k, count, 3, 64, st)
    assert want[0][0] == (0, 0, 0, 0) and st["candidates"] > st["searched"] == 1 and [r[1:5] for r in want[1]] == [(p, 6, 6, h2[p:p + 6].decode())]
    t = table_of(KT, k, reads)
    check(t, [contig, h1], 3, 64, want, "weak")
    wantc = restate_compound([contig], k, count, 3, 64)
    assert [r[1:5] for r in wantc[1]] == [(p + 2, 2, 2, h1[p + 2:p + 4].decode())]
    assert t.compound_scan([contig], 3, 64).record_tuples() == wantc[1]
    t.close()


def test_an_n_byte_and_the_end_of_the_contig_bound_r_max(KT):
    """a pair at p and p + 6 needs the bytes up to p + 6 + k - 1 to be bases: an N there, or the contig's end, takes the record away; one
    byte further on it is listed"""
    k = 31
    rng = np.random.default_rng(777)
    h1 = rand_bases(rng, 13000)
    ps = [3000, 6000, 9000]
    h2 = substitute(h1, [q for p in ps for q in (p, p + 6)])
    reads = [h1] * 5 + [h2] * 5
    count = dict_counter(kmer_dict(reads, k))
    a = bytearray(h1)
    a[ps[0] + 6 + k - 1] = ord("N")                       # inside G of R = 7
    a[ps[1] + 6 + k] = ord("n")                           # just past it
    a[ps[2] - k] = ord("N")                               # just before F
    seqs = [bytes(a), h1[:ps[2] + 6 + k - 1], h1[:ps[2] + 6 + k], h1[ps[0] - k + 1:ps[0] + 7 + k], h1[ps[0] - k + 2:ps[0] + 7 + k]]
    want = restate_clusters(seqs, k, count, 3, 64)
    assert [(r[0], r[1]) for r in want[1]] == [(0, ps[1]), (0, ps[2]), (1, ps[0]), (1, ps[1]), (2, ps[0]), (2, ps[1]), (2, ps[2]), (3, k - 1)]
    assert want[0][4] == (0, 0, 0, 0)                     # (no window before the first difference: no candidate)
    t = table_of(KT, k, reads)
    check(t, seqs, 3, 64, want, "bounds")
    check(t, seqs, 3, 7, restate_clusters(seqs, k, count, 3, 7), "bounds, 7")
    t.close()


# ---- tiles and several sequences ---------------------------------------------------------------------------------------------------
_small = {}


def small_expected(k=37, thre=3, N=64):
    """(reads, seqs, restatement), computed once: five copies of two haplotypes of 14000 bases that differ by clusters every 350 bases
    -- pairs and triples of SNPs, a SNP beside an insertion or a deletion -- two of them across the tile edges at windows 4096 and 8192;
    the sequences: both haplotypes, lower case, empty and short ones, pieces at odd offsets, one with an N"""
    key = (k, thre, N)
    if key not in _small:
        rng = np.random.default_rng(377)
        h1 = rand_bases(rng, 14000)
        at, ev = [], []
        starts = list(range(200, 13600, 350)) + [TILE + k - 4, 2 * TILE + k - 2]
        for i, p in enumerate(sorted(starts)):
            d = (1, 5, 36, 12, 20, 2, 30, 9)[i % 8]
            at += [p, p + d] + ([p + d // 2] if i % 4 == 3 else [])
            if i % 5 == 1:
                ev.append((p + d + 3, "del", 1 + i % 3))
            if i % 5 == 2:
                ev.append((p + d + 4, "ins", rand_bases(rng, 1 + i % 4)))
        h2 = plant_strings(substitute(h1, at), ev)
        seqs = [h1, h2, h1[2000:5000].lower(), b"", h1[:2 * k - 3], h1[3001:3001 + TILE + 3 * k], h2[511:911] + b"N" + h2[912:1407], h1[:k]]
        reads = [h1] * 5 + [h2] * 5
        _small[key] = reads, seqs, restate_clusters(seqs, k, dict_counter(kmer_dict(reads, k)), thre, N)
    return _small[key]


def test_clusters_across_tile_edges_and_several_sequences(KT):
    reads, seqs, want = small_expected()
    k = 37
    recs0 = [r for r in want[1] if r[0] == 0]
    assert len(recs0) >= 35 and any(r[2] != r[3] for r in recs0)
    for edge in (TILE, 2 * TILE):                         # a record whose first windows lie in one tile and whose last in the next
        assert any(r[1] - k + 1 < edge <= r[1] + r[2] - 1 for r in recs0)
    assert want[0][3] == want[0][4] == want[0][7] == (0, 0, 0, 0) and want[0][2][2] > 0 and want[0][5][2] > 0 and want[0][6][2] > 0
    assert all(c[3] == 0 for c in want[0])
    t = table_of(KT, k, reads)
    isc = check(t, seqs, 3, 64, want, "small")
    assert not isc.clusters.retried
    # the rest of the result is the scan's without clusters, with and without the mixed half
    plain, mixed = t.indel_scan(seqs, 3, 4), t.indel_scan(seqs, 3, 16, mixed=True)
    assert plain.clusters is None and mixed.clusters is None
    assert isc == plain and isc.counts == plain.counts and isc.records.tobytes() == plain.records.tobytes() and isc.variants == plain.variants and isc.mixed is None
    both = check(t, seqs, 3, 64, want, "small, mixed", max_len=16, mixed=True)
    assert both == mixed and both.mixed == mixed.mixed and both.variants == mixed.variants
    t.close()


def test_device_text_gives_what_host_text_gives(KT):
    import torch
    reads, seqs, want = small_expected()
    t = table_of(KT, 37, reads)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = t.indel_scan_device(d, offs, 3, 4, clusters=64)
    assert got.clusters.counts == want[0] and got.clusters.record_tuples() == want[1] and got == t.indel_scan_device(d, offs, 3, 4)
    t.close()


@pytest.mark.parametrize("slots,wide", [(1 << 16, True), (1 << 22, False)])
def test_narrow_against_wide(KT, slots, wide):
    reads, seqs, want = small_expected()
    t = table_of(KT, 37, reads, slots)
    assert is_wide(t) == wide
    check(t, seqs, 3, 64, want, slots)
    t.close()


@pytest.mark.parametrize("nshard", [2, 3])
def test_scan_through_owner_shards_equals_whole_table(KT, nshard):
    from test_gpu_shard import make_shards
    reads, seqs, want = small_expected()
    full = table_of(KT, 37, reads, 1 << 21)
    shards, _ = make_shards(KT, full, nshard, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    whole = check(full, seqs, 3, 64, want, "whole")
    for t in shards:
        got = t.indel_scan(seqs, 3, 4, clusters=64)
        assert got == whole and got.clusters == whole.clusters
    for t in shards + [full]:
        t.close()


def test_ten_calls_give_identical_results_and_leave_the_table_alone(KT):
    reads, seqs, want = small_expected()
    t = table_of(KT, 37, reads)
    before = t.info(), list(t.histogram())
    first = check(t, seqs, 3, 64, want, "first")
    comp = t.compound_scan(seqs, 3, 64)
    for i in range(9):
        got = t.indel_scan(seqs, 3, 4, clusters=64)
        assert got == first and got.clusters == first.clusters and got.clusters.lookups == first.clusters.lookups
        if i == 4:
            assert t.compound_scan(seqs, 3, 64) == comp and t.indel_scan(seqs[:2], 3, 4, clusters=4).clusters.counts == restate_clusters(
                seqs[:2], 37, dict_counter(kmer_dict(reads, 37)), 3, 4)[0]
    assert (t.info(), list(t.histogram())) == before
    t.close()


# ---- small k -----------------------------------------------------------------------------------------------------------------------
def k5_workload():
    """k = 5: two haplotypes of 100 bases, the second with 38 other bases in place of 40; in so small a k-mer space the walks branch and
    come back, records reach 64 bases on both sides, and from t = 5 on a window holds nothing of F"""
    from test_gpu_compound import one_way_walk
    rng = np.random.default_rng(5002)
    w = one_way_walk(rng, 100, 5)
    h2 = w[:30] + rand_bases(rng, 38) + w[70:]
    return [w] * 5 + [h2] * 5, [w, h2]


def test_k5_with_records_of_64_bases(KT):
    reads, seqs = k5_workload()
    count = dict_counter(kmer_dict(reads, 5))
    st = {}
    want = restate_clusters(seqs, 5, count, 3, 64, st)
    assert max(r[3] for r in want[1]) == 64 and max(r[2] for r in want[1]) == 64 and st["widest"] == FRONT and st["complex"] > 0 and len(want[1]) > 2000
    t = table_of(KT, 5, reads)
    check(t, seqs, 3, 64, want, "k5")
    check(t, seqs, 3, 63, restate_clusters(seqs, 5, count, 3, 63), "k5, 63")
    t.close()


def test_more_records_than_the_first_list(KT):
    """280 random bases at k = 5 and thre 1: far more records than candidates + 4096, so the search is repeated with the counted room"""
    reads, seqs = dense_workload()
    count = dict_counter(kmer_dict(reads, 5))
    st = {}
    want = restate_clusters(seqs, 5, count, 1, 64, st)
    assert len(want[1]) > 2 * (st["candidates"] + 4096) and st["complex"] > 0
    t = table_of(KT, 5, reads)
    isc = check(t, seqs, 1, 64, want, "dense")
    assert isc.clusters.retried
    assert not check(t, seqs, 1, 2, restate_clusters(seqs, 5, count, 1, 2), "dense, short").clusters.retried
    t.close()


# ---- the cap -----------------------------------------------------------------------------------------------------------------------
def fan_workload(k=21, seed=2100):
    """reads in which one candidate fans out: a contig, and 64 reads that leave it at p with the same other base x, share 5 bases and
    then hold each of the 64 strings of 3 bases and a tail of their own; `extra` is one more read that leaves one of the tails at its
    third base -- with it a level of FRONT + 1 prefixes.  -> (contig, reads, extra, p)"""
    rng = np.random.default_rng(seed)
    contig = rand_bases(rng, 12000)
    p = 6000
    x = ACGT[(ACGT.index(contig[p]) + 1) & 3]
    stem = contig[p - 40:p] + bytes([x]) + rand_bases(rng, 5)
    fans = []
    for w in range(64):
        fans.append(stem + bytes(ACGT[(w >> s) & 3] for s in (4, 2, 0)) + rand_bases(rng, 40))
    f0 = fans[0]
    cut = len(stem) + 3 + 2                                # y of that read: 1 + 5 + 3 + 2 = 11 bases
    extra = f0[:cut] + bytes([ACGT[(ACGT.index(f0[cut]) + 1) & 3]]) + rand_bases(rng, 40)
    return contig, [contig] + fans, extra, p


def test_front_plus_one_branches(KT):
    k = 21
    contig, reads, extra, p = fan_workload(k)
    for rd, cx in ((reads, 0), (reads + [extra], 1)):
        count = dict_counter(kmer_dict(rd, k))
        st = {}
        want = restate_clusters([contig], k, count, 1, 64, st)
        assert want == ([(1, 0, 0, cx)], []) and max(st["levels"]) == FRONT + cx and st["widest"] == FRONT
        t = table_of(KT, k, rd)
        check(t, [contig], 1, 64, want, cx)
        w11 = restate_clusters([contig], k, count, 1, 11)       # the level of FRONT + 1 is the twelfth: N = 11 does not reach it
        assert w11 == ([(1, 0, 0, 0)], [])
        check(t, [contig], 1, 11, w11, (cx, 11))
        t.close()


def test_the_cap_at_k4(KT):
    """test_het_clusters_host.cap_workload: with N = 5 every level fits, with N = 6 some candidates are complex and keep their shorter
    records"""
    reads, seqs = cap_workload()
    count = dict_counter(kmer_dict(reads, 4))
    t = table_of(KT, 4, reads)
    for N in (5, 6, 64):
        want = restate_clusters(seqs, 4, count, 1, N)
        assert (want[0][0][3] > 0) == (N > 5)
        check(t, seqs, 1, N, want, N)
    t.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_an_empty_table_gives_nothing(KT):
    _, seqs, _ = small_expected()
    zeros = [(0, 0, 0, 0)] * len(seqs)
    empty = KT(31, min_slots=1 << 16)
    for _ in range(2):
        isc = check(empty, seqs, 1, 64, (zeros, []), "empty")
        assert not isc.clusters.retried and isc.clusters.lookups == 0
        empty.count_bases(seqs[0])
        empty.clear()
    hc = empty.indel_scan([], 1, clusters=64).clusters
    assert hc.counts == [] and len(hc.records) == 0
    assert empty.indel_scan(["", "ACG"], 1, clusters=1).clusters.counts == [(0, 0, 0, 0)] * 2
    empty.close()


def test_bad_arguments_are_errors(KT):
    import ctypes as C
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.indel_scan(s, 0, clusters=64)
        with pytest.raises(_lib.JasperHipError, match="max_len"):
            t.indel_scan(s, 1, 17, clusters=64)
        for bad in (65, -1, 1000):
            with pytest.raises(_lib.JasperHipError, match="cluster_len"):
                t.indel_scan(s, 1, clusters=bad)
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    ln = (C.c_int64 * 1)(200)
    res = C.c_void_p()
    for n in (1, 0):
        assert L.jasper_indel_scan_clusters(t._h, n, cs, ln, 1, 4, 0, 0, C.byref(res)) != 0 and not res
        assert b"cluster_len" in L.jasper_last_error()
    assert L.jasper_indel_scan_clusters(t._h, 1, cs, ln, 1, 4, 0, 4, None) != 0
    assert L.jasper_indel_scan_clusters(None, 1, cs, ln, 1, 4, 0, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indel_scan_clusters_device(t._h, 1, None, None, 1, 4, 0, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indelscan_cluster_counts(None, 0, None) != 0 and L.jasper_indelscan_cluster_records(None, None, None) != 0
    assert L.jasper_indelscan_cluster_lookups(None, None) != 0 and L.jasper_indelscan_cluster_seconds(None) == 0.0 and L.jasper_indelscan_cluster_retried(None) == 0
    # a result of the entry point without clusters: zeros and n = 0
    assert L.jasper_indel_scan(t._h, 1, cs, ln, 1, 4, C.byref(res)) == 0 and res
    c4 = (C.c_uint64 * 4)(9, 9, 9, 9)
    rp, rn, nl = C.POINTER(_lib.HetCluster)(), C.c_uint64(7), C.c_uint64(7)
    assert L.jasper_indelscan_cluster_counts(res, 0, c4) == 0 and list(c4) == [0, 0, 0, 0] and L.jasper_indelscan_cluster_counts(res, 1, c4) != 0
    assert L.jasper_indelscan_cluster_records(res, C.byref(rp), C.byref(rn)) == 0 and rn.value == 0
    assert L.jasper_indelscan_cluster_lookups(res, C.byref(nl)) == 0 and nl.value == 0
    assert L.jasper_indelscan_cluster_seconds(res) == 0.0 and L.jasper_indelscan_cluster_retried(res) == 0
    L.jasper_indelscan_free(res)
    t1 = KT(1, min_slots=1 << 16)
    with pytest.raises(_lib.JasperHipError, match="k must"):
        t1.indel_scan(seqs, 1, clusters=4)
    t1.close()
    count = dict_counter(kmer_dict([b"ACGT" * 100], 31))
    check(t, seqs, 1, 64, restate_clusters(seqs, 31, count, 1, 64), "a period of four")
    t.close()


# ---- noisy reads -------------------------------------------------------------------------------------------------------------------
def repeat_workload(k=37, seed=3700):
    """a genome of 14000 bases in which a unit of 1500 bases stands three times, the copies 1.5 % apart from each other, and 100-base
    reads of it at 30x with 0.3 % substitution errors, both strands: at thre 2 the other copies are the second haplotype, their
    differences less than k apart are the clusters, and coincident read errors add candidates of their own"""
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    g = bytearray(rand_bases(rng, 14000))
    unit = rand_bases(rng, 1500)
    for at in (1000, 6000, 11000):
        g[at:at + 1500] = substitute(unit, sorted(set(int(x) for x in rng.integers(0, 1500, 22))))
    g = bytes(g)
    reads = synth.make_reads_stream(rng, np.frombuffer(g, dtype=np.uint8), 30, 100, 0.003).reshape(-1, 101)[:, :100]
    return [r.tobytes() for r in reads], [g]


def test_repeat_copies_under_noisy_reads(KT):
    reads, seqs = repeat_workload()
    count = dict_counter(kmer_dict(reads, 37))
    st = {}
    want = restate_clusters(seqs, 37, count, 2, 64, st)
    assert len(want[1]) >= 10 and st["candidates"] >= st["searched"] >= 30 and len({r[3] for r in want[1]}) >= 5
    t = table_of(KT, 37, reads)
    check(t, seqs, 2, 64, want, "repeats")
    check(t, seqs, 2, 9, restate_clusters(seqs, 37, count, 2, 9), "repeats, 9")
    t.close()
