"""GPU: the compound scan (KmerTable.compound_scan / compound_scan_device, jasper_compound_scan) against the restatement of its semantics
in test_compound_host.py, fed by Python dicts of canonical k-mer strings.  Nothing expected here comes from the code under test.  Every
workload also states that the embedded report is kmer_report's."""
import numpy as np
import pytest

from golden_util import Case, case_names
from test_compound_host import COMPOUND_ANCHORS, FRONT, cap_workload, planted_pairs, restate_compound, substitute
from test_gpu_copies import TILE, dict_counter, is_wide, kmer_dict
from test_indels_host import ACGT, rand_bases
from test_indels_mixed_host import plant_strings, random_string

pytestmark = pytest.mark.gpu


def check(t, seqs, thre, max_len, want, what):
    """compound_scan against (counts, records) of the restatement; its report against kmer_report"""
    cs = t.compound_scan(seqs, thre, max_len)
    assert cs.counts == want[0], what
    got = cs.record_tuples()
    assert len(got) == len(want[1]), (what, len(got), len(want[1]))
    assert got == want[1], what
    assert all(bytes(r["pad"]) == bytes(6) for r in cs.records[:100])
    assert cs.report == t.kmer_report(seqs, thre), what
    assert 0 <= cs.search_seconds <= cs.seconds
    return cs


def table_of(KT, k, reads, min_slots=1 << 16):
    t = KT(k, min_slots=min_slots)
    t.count_bases(b"N".join(reads))
    return t


def applied(contig, recs):
    """the contig with its records put in place of what they replace (one record per site)"""
    out = bytearray(contig)
    assert len({r[1] for r in recs}) == len(recs)
    for _, pos, rlen, _, y, _, _ in sorted(recs, key=lambda r: -r[1]):
        out[pos:pos + rlen] = y.encode()
    return bytes(out)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE and KmerTable.compound_front() == FRONT
    return KmerTable


# ---- golden cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    want64, want4 = restate_compound(seqs, c.k, count, c.thre, 64), restate_compound(seqs, c.k, count, c.thre, 4)
    assert len(want64[1]) == COMPOUND_ANCHORS.get(name, (0, 0, 0))[0]
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    cs = check(t, seqs, c.thre, 64, want64, name)
    check(t, seqs, c.thre, 4, want4, (name, 4))
    t.close()
    assert not cs.retried and (cs.lookups > 0) == (sum(x[0] for x in want64[0]) > 0)


# ---- planted pairs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31, 64])
def test_planted_pairs(KT, k):
    """pairs of substitutions 1, 2, 3, 7, k-2, k-1 and k apart (one record each, y = the truth; at k = 64 and d = 64 the run is long), a
    pair k + 3 apart (two sites with R = 1: nothing listed) -- test_compound_host.test_planted_pairs states the same of the restatement"""
    truth, contig, pairs, far = planted_pairs(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    want = restate_compound([contig], k, count, 3, 64)
    assert [(r[1], r[2], r[3], r[4]) for r in want[1]] == [(p, d + 1, d + 1, truth[p:p + d + 1].decode()) for p, d in pairs if d < 64]
    assert want[0] == [(len(want[1]) + 2, len(want[1]), len(want[1]), 1 if k == 64 else 0, 0)]
    t = table_of(KT, k, [truth] * 5)
    check(t, [contig], 3, 64, want, k)
    # R exactly max_len is listed, R = max_len + 1 is long
    for max_len in (8, 7):
        w = restate_compound([contig], k, count, 3, max_len)
        assert ((pairs[3][0], 8, 8) in [(r[1], r[2], r[3]) for r in w[1]]) == (max_len == 8) and w[0][0][3] == (3 if max_len == 8 else 4)
        check(t, [contig], 3, max_len, w, (k, max_len))
    t.close()


def indel_clusters(k, seed=66):
    """(truth, contig): the truth with, in the contig, a substitution 5 bases before 2 bytes that the contig lacks, and another 5 bases
    before 3 mixed bases that only the contig holds"""
    rng = np.random.default_rng(seed + k)
    truth = rand_bases(rng, 12 * k)
    p1, p2 = 3 * k, 8 * k
    c = substitute(truth, [p1, p2])
    ins = random_string(rng, 3, not_first=truth[p2 + 6])
    return truth, plant_strings(c, [(p1 + 6, "del", 2), (p2 + 6, "ins", ins)])


@pytest.mark.parametrize("k", [21, 31, 64])
def test_a_substitution_next_to_a_length_error(KT, k):
    truth, contig = indel_clusters(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    want = restate_compound([contig], k, count, 3, 64)
    assert want[0] == [(2, 2, 2, 0, 0)] and [r[3] - r[2] for r in want[1]] == [2, -3]      # both complex: R != t
    assert applied(contig, want[1]) == truth
    t = table_of(KT, k, [truth] * 5)
    check(t, [contig], 3, 64, want, k)
    t.close()


# ---- the shift boundaries ----------------------------------------------------------------------------------------------------------
def one_way_walk(rng, n, k):
    """n random bases in which every (k-1)-mer occurs once, counting both strands, and none is its own reverse complement: from any
    k - 1 bases of it the k-mers of the string lead one way only"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    while True:
        s = bytearray(rand_bases(rng, k - 2))
        seen = set()
        while len(s) < n:
            for z in rng.permutation(4):
                m = bytes(s[len(s) - (k - 2):]) + ACGT[z:z + 1]
                rc = m.translate(comp)[::-1]
                if m != rc and m not in seen and rc not in seen:
                    seen.add(m)
                    s.append(ACGT[z])
                    break
            else:
                break
        if len(s) == n:
            return bytes(s)


def long_site_k5():
    """k = 5: a truth of 84 bases whose 5-mers lead one way only, and a contig in which 64 of them are replaced by bases chosen so that
    no window that holds one is a 5-mer of the truth -- one site with R = 64 whose record of 64 bases is the truth.  From t = 5 on a
    window holds nothing of F."""
    k = 5
    rng = np.random.default_rng(4005)
    truth = one_way_walk(rng, 84, k)
    solid = kmer_dict([truth], k)
    count = dict_counter(solid)
    while True:
        c = bytearray(truth)
        for i in range(10, 74):
            free = [z for z in rng.permutation(4) if not count(bytes(c[i - 4:i]) + ACGT[z:z + 1])]
            if not free:
                break
            c[i] = ACGT[free[0]]
        else:
            if not any(count(bytes(c[i:i + k])) for i in range(70, 74)):
                return k, truth, bytes(c)


def test_len_64_at_k5(KT):
    k, truth, contig = long_site_k5()
    count = dict_counter(kmer_dict([truth] * 5, k))
    st = {}
    want = restate_compound([contig], k, count, 3, 64, st)
    assert want == ([(1, 1, 1, 0, 0)], [(0, 10, 64, 64, truth[10:74].decode(), 0, 5)]) and st["levels"] == [1] * 64
    want63 = restate_compound([contig], k, count, 3, 63)
    assert want63 == ([(0, 0, 0, 1, 0)], [])                 # R = max_len + 1: long
    t = table_of(KT, k, [truth] * 5)
    check(t, [contig], 3, 64, want, "k5")
    check(t, [contig], 3, 63, want63, "k5, 63")
    t.close()


def test_len_64_at_k64(KT):
    """at k = 64 the pair 63 apart is a record of exactly 64 bases: F << 2t runs up to 126 bits, and at t = 64 = k it is not formed"""
    truth, contig, pairs, _ = planted_pairs(64)
    count = dict_counter(kmer_dict([truth] * 5, 64))
    want = restate_compound([contig], 64, count, 3, 64)
    assert (pairs[5][0], 64, 64, truth[pairs[5][0]:pairs[5][0] + 64].decode()) in [(r[1], r[2], r[3], r[4]) for r in want[1]]
    # a second contig whose reads hold 64 bases where it holds 60: t = 64 > R
    rng = np.random.default_rng(640)
    g = rand_bases(rng, 400)
    c2 = plant_strings(substitute(g, [150, 213]), [(180, "del", 4)])
    count2 = dict_counter(kmer_dict([truth] * 5 + [g] * 5, 64))
    want2 = restate_compound([contig, c2], 64, count2, 3, 64)
    assert want2[1][-1][:5] == (1, 150, 60, 64, g[150:214].decode()) and want2[0][1] == (1, 1, 1, 0, 0)
    t = table_of(KT, 64, [truth] * 5 + [g] * 5)
    check(t, [contig, c2], 3, 64, want2, "k64")
    t.close()


# ---- edges -------------------------------------------------------------------------------------------------------------------------
def edges_workload(k=31):
    rng = np.random.default_rng(3100)
    truth = rand_bases(rng, 3000)
    a = truth[:600]
    c0 = substitute(a, [k - 1, k + 2, 300, 303, 600 - k - 3, 600 - k])      # a run from window 0, one in the middle, one to the last window
    b = bytearray(substitute(truth[700:1300], [300, 304]))
    b[300 - k] = ord("N")                                                     # the byte before F and the byte after G
    b[304 + k] = ord("N")
    c2 = substitute(truth[1400:2000], [200, 207, 213]).lower()
    c3 = substitute(truth[2100:2500], [200])                                  # R = 1 and a solid substitution: the variant scan's
    seqs = [c0, bytes(b), c2, c3, truth[:k - 1], b"", substitute(truth[2500:2900], [100, 100 + k - 1])]
    want_recs = [(0, k - 1, 4, 4, a[k - 1:k + 3].decode(), 0, 5), (0, 300, 4, 4, a[300:304].decode(), 0, 5),
                 (0, 600 - k - 3, 4, 4, a[600 - k - 3:600 - k + 1].decode(), 0, 5),
                 (1, 300, 5, 5, truth[1000:1005].decode(), 0, 5), (2, 200, 14, 14, truth[1600:1614].decode(), 0, 5),
                 (6, 100, k, k, truth[2600:2600 + k].decode(), 0, 5)]
    want_counts = [(3, 3, 3, 0, 0), (1, 1, 1, 0, 0), (1, 1, 1, 0, 0), (1, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (1, 1, 1, 0, 0)]
    return k, [truth] * 5, seqs, (want_counts, want_recs)


def test_edges(KT):
    k, reads, seqs, want = edges_workload()
    assert restate_compound(seqs, k, dict_counter(kmer_dict(reads, k)), 3, 64) == want
    t = table_of(KT, k, reads)
    check(t, seqs, 3, 64, want, "edges")
    t.close()


# ---- the cap -----------------------------------------------------------------------------------------------------------------------
def test_the_cap(KT):
    """test_compound_host.cap_workload: a level of exactly 64 prefixes is searched and listed whole, the next one of 155 makes the site
    complex once and leaves the shorter records"""
    reads, seqs = cap_workload()
    count = dict_counter(kmer_dict(reads, 4))
    st = {}
    want5, want6 = restate_compound(seqs, 4, count, 1, 5), restate_compound(seqs, 4, count, 1, 6, st)
    assert want5[0] == [(1, 1, 41, 0, 0)] and want6[0] == [(1, 1, 41, 0, 1)] and st["levels"][-2:] == [FRONT, 155] and want5[1] == want6[1]
    t = table_of(KT, 4, reads)
    check(t, seqs, 1, 5, want5, "fits")
    check(t, seqs, 1, 6, want6, "complex")
    check(t, seqs, 1, 64, want6, "complex, 64")
    t.close()


def dense_workload():
    """k = 4 and thre 24 on 3000 random bases of reads (a 4-mer is there 22 times on average): about half of all 4-mers are solid, so a
    contig of random bases is full of runs and a site has a dozen records before its level passes 64"""
    rng = np.random.default_rng(44)
    return [rand_bases(rng, 3000)], [rand_bases(rng, 15000), rand_bases(rng, 3000)]


def test_more_records_than_the_first_list(KT):
    reads, seqs = dense_workload()
    count = dict_counter(kmer_dict(reads, 4))
    st = {}
    want = restate_compound(seqs, 4, count, 24, 64, st)
    assert len(want[1]) > 2 * (st["sites"] + 4096) and st["complex"] > 0 and st["longest"] > 4
    t = table_of(KT, 4, reads)
    cs = check(t, seqs, 24, 64, want, "dense")
    assert cs.retried
    assert not check(t, seqs[1:], 24, 2, restate_compound(seqs[1:], 4, count, 24, 2), "dense, short").retried
    t.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
FUZZ = {5: (84, 2, 90), 6: (300, 2, 12), 21: (6000, 2, 2), 37: (6000, 2, 2)}      # k: genome bases, thre, derived contigs


def fuzz_workload(k, seed=7300):
    """random reads of 100 bases at low coverage (8x, so the reads themselves leave gaps) over a random genome, and contigs derived from
    it (for k >= 21 the reads come from two haplotypes): clusters of two or three substitutions, a substitution next to an insertion or a deletion, an N, lower case, short pieces.  At
    k = 5 and 6 the genome is a one-way walk: in plain random bases every (k-1)-mer comes back, the graph of the reads is full of
    cycles and at max_len 64 every site is complex"""
    G, thre, ncontigs = FUZZ[k]
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, G) if k >= 21 else one_way_walk(rng, G, k)
    h = substitute(g, range(17, G, 40)) if k >= 21 else g        # a second haplotype: the walks branch at its differences
    rl = min(100, G // 2)
    reads = [(g, h)[i & 1][s:s + rl] for i, s in enumerate(int(rng.integers(0, G - rl + 1)) for _ in range(8 * G // rl))]
    seqs = []
    for c in range(ncontigs):
        b, ev = bytearray(g), []
        step = 2 * k + 9 if k >= 21 else k + 8
        for i, p in enumerate(range(step + c, G - step, step)):
            kind = int(rng.integers(0, 5))
            d = int(rng.integers(1, max(2, min(k, 30))))
            at = [p, p + d] + ([p + d // 2] if kind == 1 and d > 1 else [])
            for x in at:
                b[x] = ACGT[(ACGT.index(b[x]) + 1 + int(rng.integers(0, 3))) & 3]
            if kind == 2:
                ev.append((p + d + 1, "del", int(rng.integers(1, 4))))
            if kind == 3:
                ev.append((p + d + 1, "ins", rand_bases(rng, int(rng.integers(1, 4)))))
        seqs.append(plant_strings(bytes(b), ev))
    a = bytearray(seqs[0])
    a[len(a) // 2] = ord("N")
    seqs += [bytes(a), seqs[-1][: len(seqs[-1]) // 2].lower(), g[:k - 1], b"", g[: 2 * k]]
    return reads, seqs, thre


@pytest.mark.parametrize("k", sorted(FUZZ))
def test_fuzz_against_dicts(KT, k):
    reads, seqs, thre = fuzz_workload(k)
    count = dict_counter(kmer_dict(reads, k))
    t = table_of(KT, k, reads)
    for max_len in (64, 5):
        st = {}
        want = restate_compound(seqs, k, count, thre, max_len, st)
        print(k, max_len, [sum(c[i] for c in want[0]) for i in range(5)], st["widest"], st["longest"])
        if max_len == 64:                                     # conditions on the input, from the restatement alone
            assert len(want[1]) >= 50 and 10 * st["complex"] <= st["sites"] and st["long"] + st["sites"] > sum(c[1] for c in want[0])
        check(t, seqs, thre, max_len, want, (k, max_len))
    t.close()


def test_device_text_gives_what_host_text_gives(KT):
    import torch
    reads, seqs, thre = fuzz_workload(37)
    t = table_of(KT, 37, reads)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    cs = t.compound_scan(seqs, thre, 64)
    assert len(cs.records) >= 50 and t.compound_scan_device(d, offs, thre, 64) == cs
    t.close()


# ---- table shapes ------------------------------------------------------------------------------------------------------------------
_small = {}


def small_expected(k=37, thre=3, max_len=64):
    """(reads, seqs, restatement), computed once: five copies of a genome, and an assembly with a cluster every 150 bases"""
    key = (k, thre, max_len)
    if key not in _small:
        rng = np.random.default_rng(377)
        g = rand_bases(rng, 8000)
        ev, at = [], []
        for i, p in enumerate(range(200, 7800, 150)):
            d = (1, 5, 36, 12, 37, 2, 30, 40)[i % 8]
            at += [p, p + d] + ([p + 60, p + 75] if i % 8 == 6 else [])      # (four of them, 76 bytes end to end: a long run)
            if i % 3 == 1:
                ev.append((p + d + 3, "del", 1 + i % 4))
            if i % 3 == 2:
                ev.append((p + d + 2, "ins", random_string(rng, 1 + i % 5)))
        asm = plant_strings(substitute(g, at), ev)
        seqs = [asm, asm[2000:5000].lower(), b"", asm[:2 * k - 3], asm[3000:3000 + TILE + 3 * k], asm[500:900] + b"N" + asm[901:1400]]
        reads = [g] * 5
        _small[key] = reads, seqs, restate_compound(seqs, k, dict_counter(kmer_dict(reads, k)), thre, max_len)
    return _small[key]


@pytest.mark.parametrize("slots,wide", [(1 << 16, True), (1 << 22, False)])
def test_narrow_against_wide(KT, slots, wide):
    reads, seqs, want = small_expected()
    assert len(want[1]) > 60 and any(r[2] != r[3] for r in want[1]) and sum(c[3] for c in want[0]) > 0
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
        assert t.compound_scan(seqs, 3, 64) == whole
    for t in shards + [full]:
        t.close()


def test_ten_calls_and_interleaved_scans_keep_their_results_and_leave_the_table_alone(KT):
    k = 37
    reads, seqs, want = small_expected()
    t = table_of(KT, k, reads)
    before = t.info(), list(t.histogram())
    first = check(t, seqs, 3, 64, want, "first")
    krep, vs, mixed = t.kmer_report(seqs, 3), t.variant_scan(seqs, 3), t.indel_scan(seqs, 3, 16, mixed=True)

    def again():
        got = t.compound_scan(seqs, 3, 64)
        assert got == first and got.lookups == first.lookups

    for _ in range(5):
        again()
    assert t.kmer_report(seqs, 3) == krep
    again()
    got = t.indel_scan(seqs, 3, 16, mixed=True)
    assert got == mixed and got.mixed == mixed.mixed
    again()
    assert t.variant_scan(seqs, 3) == vs
    again()
    assert t.compound_scan(seqs[:2], 3, 4).counts == restate_compound(seqs[:2], k, dict_counter(kmer_dict(reads, k)), 3, 4)[0]
    again()
    got = t.indel_scan(seqs, 3, 16, mixed=True)
    assert t.kmer_report(seqs, 3) == krep and t.variant_scan(seqs, 3) == vs and got == mixed and got.mixed == mixed.mixed
    assert (t.info(), list(t.histogram())) == before
    t.close()


def test_an_empty_table_gives_nothing(KT):
    """every window is unreliable: a sequence is one run, long or -- a short one -- a site that nothing bridges"""
    k = 31
    _, seqs, _ = small_expected()
    want = restate_compound(seqs, k, lambda km: 0, 1, 64)
    assert not want[1] and sum(c[0] for c in want[0]) == 1 and sum(c[3] for c in want[0]) == 5 and all(c[1] == c[2] == c[4] == 0 for c in want[0])
    empty = KT(k, min_slots=1 << 16)
    for _ in range(2):
        cs = check(empty, seqs, 1, 64, want, "empty")
        assert not cs.retried
        empty.count_bases(seqs[0])
        empty.clear()
    assert empty.compound_scan([], 1).counts == [] and empty.compound_scan(["", "ACG"], 1).counts == [(0, 0, 0, 0, 0)] * 2
    empty.close()


def test_bad_arguments_are_errors(KT):
    import ctypes as C
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.compound_scan(s, 0)
        for bad in (0, 65, -1):
            with pytest.raises(_lib.JasperHipError, match="max_len"):
                t.compound_scan(s, 1, bad)
    t1 = KT(1, min_slots=1 << 16)
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="k must"):
            t1.compound_scan(s, 1)
    t1.close()
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    res = C.c_void_p()
    assert L.jasper_compound_scan(t._h, 1, cs, (C.c_int64 * 1)(-5), 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_compound_scan(t._h, 1, cs, (C.c_int64 * 1)(200), 1, 4, None) != 0
    assert L.jasper_compound_scan(None, 1, cs, (C.c_int64 * 1)(200), 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_compound_scan_device(t._h, 1, None, None, 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_compscan_counts(None, 0, None) != 0 and L.jasper_compscan_records(None, None, None) != 0 and L.jasper_compscan_seconds(None, None, None) != 0
    assert L.jasper_compound_scan(t._h, 1, cs, (C.c_int64 * 1)(200), 1, 4, C.byref(res)) == 0 and res
    c5 = (C.c_uint64 * 5)()
    assert L.jasper_compscan_counts(res, 0, c5) == 0 and L.jasper_compscan_counts(res, 1, c5) != 0 and L.jasper_compscan_num_seqs(res) == 1
    assert L.jasper_report_num_seqs(L.jasper_compscan_report(res)) == 1
    L.jasper_compscan_free(res)
    count = dict_counter(kmer_dict([b"ACGT" * 100], 31))
    check(t, seqs, 1, 64, restate_compound(seqs, 31, count, 1, 64), "a period of four")
    t.close()
