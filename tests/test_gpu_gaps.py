"""GPU: the gap scan (KmerTable.gap_scan / gap_scan_device / gap_search, jasper_gap_scan) against the restatement of its semantics in
test_gaps_host.py, fed by Python dicts of canonical k-mer strings.  Nothing expected here comes from the code under test.  Every
workload also states that the embedded report is kmer_report's.  The workloads (functions named *_workload) state what they are about
on the restatement alone, so they can be checked without a GPU."""
import numpy as np
import pytest

from golden_util import Case, case_names
from test_compound_host import planted_pairs, restate_compound, substitute
from test_gaps_host import FRONT, MAXREC, fill_lengths, planted_fills, repeat_workload, restate_gap_search, restate_gaps
from test_gpu_copies import TILE, dict_counter, kmer_dict
from test_indels_host import rand_bases

pytestmark = pytest.mark.gpu


def check_result(gs, want, what):
    assert gs.counts == want[0], what
    assert gs.site_tuples() == want[1], what
    got = gs.record_tuples()
    assert len(got) == len(want[2]), (what, len(got), len(want[2]))
    assert got == want[2], what
    assert all(bytes(s["pad"]) == bytes(6) for s in gs.sites)
    assert len(gs.bases) == sum(r[3] for r in want[2]) and 0 <= gs.search_seconds <= gs.seconds


def check(t, seqs, thre, max_len, max_trim, long_runs, want, what):
    """gap_scan against (counts, sites, records) of the restatement; its report against kmer_report"""
    gs = t.gap_scan(seqs, thre, max_len, max_trim, long_runs)
    check_result(gs, want, what)
    assert gs.report == t.kmer_report(seqs, thre), what
    return gs


def table_of(KT, k, reads, min_slots=1 << 16):
    t = KT(k, min_slots=min_slots)
    t.count_bases(b"N".join(reads))
    return t


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE and KmerTable.gap_front() == FRONT and KmerTable.gap_max_records() == MAXREC and KmerTable.gap_max_len() == 4096
    return KmerTable


# ---- golden cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    for long_runs in (True, False):
        check(t, seqs, c.thre, 200, c.k, long_runs, restate_gaps(seqs, c.k, count, c.thre, 200, c.k, long_runs), (name, long_runs))
    t.close()


# ---- planted fills -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32, 64])
def test_planted_fills(KT, k):
    """fills of 0, 1, k-2, k-1, k, 63, 64, 65, 127, 128 and 129 bases behind N runs of other lengths, in one contig: each is listed once
    and is the truth -- test_gaps_host.test_planted_fills states the same of the restatement"""
    from jasper_amd import gaps
    truth, contig, plants = planted_fills(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    want = restate_gaps([contig], k, count, 3, 200, k, False)
    assert [(r[1], r[2], r[3], r[4]) for r in want[2]] == [(a, nn, L, truth[p:p + L].decode()) for a, nn, L, p in plants] and [L for _, _, L, _ in plants] == fill_lengths(k)
    t = table_of(KT, k, [truth] * 5)
    gs = check(t, [contig], 3, 200, k, False, want, k)
    filled = gaps.fill_sequences([contig], gs.sites, gs.record_tuples())
    assert filled == [truth]
    rep = t.kmer_report(filled, 3)
    assert rep.counts[0][2] == 0 and len(rep.runs) == 0                 # the filled text has no unreliable window
    # one of them alone, with the limit on either side of its length
    truth1, contig1, ((a, nn, L, p),) = planted_fills(k, [65], seed=3)
    count1 = dict_counter(kmer_dict([truth1] * 5, k))
    t1 = table_of(KT, k, [truth1] * 5)
    for max_len, nrec in ((65, 1), (64, 0)):
        w = restate_gaps([contig1], k, count1, 3, max_len, k, False)
        assert w[1] == [(0, a, a + nn, "gap", "limit", nrec, max_len, 0, 0, 0)] and len(w[2]) == nrec
        check(t1, [contig1], 3, max_len, k, False, w, (k, max_len))
    for x in (t, t1):
        x.close()


def test_a_walk_of_4096_levels(KT):
    """one fill of 4096 bases at k = 21: listed at max_len 4096, limit without a record at 4095"""
    k = 21
    truth, contig, ((a, nn, L, p),) = planted_fills(k, [4096], seed=4096)
    count = dict_counter(kmer_dict([truth] * 5, k))
    t = table_of(KT, k, [truth] * 5)
    for max_len, recs in ((4096, [(0, a, nn, 4096, truth[p:p + 4096].decode(), 0, 5)]), (4095, [])):
        want = restate_gaps([contig], k, count, 3, max_len, k, False)
        assert want[1] == [(0, a, a + nn, "gap", "limit", len(recs), max_len, 0, 0, 0)] and want[2] == recs
        check(t, [contig], 3, max_len, k, False, want, max_len)
    t.close()


# ---- slots that move ---------------------------------------------------------------------------------------------------------------
def moving_slots_workload(k=21, seed=9):
    """(reads, contig, want): a fill of 40 bases that the reads hold in two alleles, and reads that leave the true path at base `off` of
    the fill with an A where the truth has another base and end 4 bases later.  That spur sorts before the true path, so for five levels
    the true path is in slot 1; then the spur has no extension, the front is compacted and the true path is back in slot 0: the log's
    parent slots are not the identity.  Both strings must come back exact."""
    rng = np.random.default_rng(seed)
    truth = rand_bases(rng, 8 * k + 40)
    a, L = 4 * k, 40
    off = next(i for i in range(8, 20) if truth[a + i:a + i + 1] != b"A")
    spur = truth[a + off - (k - 1):a + off] + b"A" + rand_bases(rng, 4)
    hap2 = substitute(truth, [a + 30])
    reads = [truth] * 5 + [hap2] * 5 + [spur] * 5
    contig = truth[:a] + b"N" * 7 + truth[a + L:]
    st = {}
    want = restate_gaps([contig], k, dict_counter(kmer_dict(reads, k)), 3, 200, k, False, st)
    lv = st["levels"][0]
    assert lv[:off] == [1] * off and lv[off:off + 5] == [2] * 5 and lv[off + 5:30] == [1] * (25 - off) and lv[30:L + k - 1] == [2] * (L + k - 31)
    assert [(r[3], r[4]) for r in want[2]] == sorted((L, h[a:a + L].decode()) for h in (truth, hap2)) and want[0] == [(1, 1, 1, 0, 2, 0, 0, 0, 0)]
    return reads, contig, want


def test_slots_that_move(KT):
    from jasper_amd import gaps
    reads, contig, want = moving_slots_workload()
    t = table_of(KT, 21, reads)
    gs = check(t, [contig], 3, 200, 21, False, want, "moving slots")
    assert gaps.fill_sequences([contig], gs.sites, gs.record_tuples()) == [contig]      # two records: not unique, not filled
    t.close()


# ---- the front and the record cap ----------------------------------------------------------------------------------------------------
def front_workload():
    """(reads, contigs, (max_len that fits, its restatement), (the next, its restatement)) at k = 4 and thre 1, in the manner of
    test_compound_host.cap_workload: one read of 90 random bases and a contig cut from it with two Ns.  Its levels hold 2, 6, 14, 29, 64
    and 156 strings: at max_len 5 the front just fits, at 6 the site is complex and keeps its shorter records."""
    rng = np.random.default_rng(787)
    g = rand_bases(rng, 90)
    lo = int(rng.integers(10, 90 - 50))
    c = bytearray(g[lo:lo + 40])
    c[18:21] = b"NN"
    count = dict_counter(kmer_dict([g], 4))
    st5, st6 = {}, {}
    want5, want6 = restate_gaps([bytes(c)], 4, count, 1, 5, 4, False, st5), restate_gaps([bytes(c)], 4, count, 1, 6, 4, False, st6)
    assert st5["levels"] == [[2, 6, 14, 29, FRONT]] and st6["levels"] == [[2, 6, 14, 29, FRONT, 156]]
    assert want5[1][0][4:7] == ("limit", len(want5[2]), 5) and want6[1][0][4:7] == ("complex", len(want5[2]), 6) and want5[2] == want6[2]
    assert 0 < len(want5[2]) <= MAXREC and max(r[3] for r in want5[2]) == 5
    return [g], [bytes(c)], (5, want5), (6, want6)


def test_the_front(KT):
    reads, seqs, fits, passes = front_workload()
    t = table_of(KT, 4, reads)
    check(t, seqs, 1, fits[0], 4, False, fits[1], "fits")
    check(t, seqs, 1, passes[0], 4, False, passes[1], "complex")
    t.close()


def test_the_record_cap(KT):
    """a site inside Ax60: lengths 0 .. 15 listed, complex at level 16; a site inside (ACG)x40: seven records, dead, not filled --
    test_gaps_host states both of the restatement"""
    from jasper_amd import gaps
    for unit, copies, status, nrec in ((b"A", 60, "complex", 16), (b"ACG", 40, "dead", 7)):
        reads, contig, a = repeat_workload(unit, copies)
        want = restate_gaps([contig], 21, dict_counter(kmer_dict(reads, 21)), 3, 200, 21, False)
        assert want[1][0][3:6] == ("gap", status, nrec) and want[0][0][3] == 0
        t = table_of(KT, 21, reads)
        gs = check(t, [contig], 3, 200, 21, False, want, unit)
        assert gaps.fill_sequences([contig], gs.sites, gs.record_tuples()) == [contig]
        t.close()


# ---- more than the first lists hold ------------------------------------------------------------------------------------------------
def retry_workload(k=21):
    """twelve fills of 4000 bases: more bytes than the first pool (2048 a site + 16384) holds"""
    truth, contig, plants = planted_fills(k, [4000] * 12, seed=12, n_runs={4000: 20})
    want = restate_gaps([contig], k, dict_counter(kmer_dict([truth] * 5, k)), 3, 4096, k, False)
    assert len(want[2]) == 12 and sum(r[3] for r in want[2]) > 2048 * 12 + 16384
    return truth, contig, want


def test_more_bytes_than_the_first_pool(KT):
    from jasper_amd import gaps
    truth, contig, want = retry_workload()
    t = table_of(KT, 21, [truth] * 5)
    gs = check(t, [contig], 3, 4096, 21, False, want, "retry")
    assert gs.retried and gaps.fill_sequences([contig], gs.sites, gs.record_tuples()) == [truth]
    short = restate_gaps([contig], 21, dict_counter(kmer_dict([truth] * 5, 21)), 3, 100, 21, False)
    assert not check(t, [contig], 3, 100, 21, False, short, "no retry").retried and not short[2]
    t.close()


# ---- explicit sites ----------------------------------------------------------------------------------------------------------------
def compound_sites(runs, k, max_len):
    """the compound scan's own sites from the report's runs: (seq, a, q, ref_min)"""
    return [(seq, start + k - 1, start + nk, mn) for seq, start, nk, _, mn in runs if nk >= k and nk - k + 1 <= max_len]


def explicit_workloads():
    out = []
    c = Case("cluster_k25")
    _, seqs = c.batch()
    out.append(("cluster_k25", c.k, c.thre, None, c.reads_text(), seqs, dict_counter({key.encode(): v for key, v in c.dump().items()})))
    for k in (21, 31, 64):
        truth, contig, _, _ = planted_pairs(k)
        out.append(("pairs %d" % k, k, 3, [truth] * 5, None, [contig], dict_counter(kmer_dict([truth] * 5, k))))
    return out


def explicit_expectation(k, thre, seqs, count, max_len=64):
    """(sites, restatement of gap_search on them, compound's records): the search on the compound scan's sites lists what it lists, but
    for the single substitutions (R = t = 1), which the compound scan leaves to the variant scan"""
    from test_gpu_kmer_report import restate as restate_runs
    from test_gpu_kmer_report import window_counts
    sites = compound_sites(restate_runs([window_counts(s, k, count) for s in seqs], thre)[1], k, max_len)
    want = restate_gap_search(seqs, k, count, thre, max_len, sites)
    comp = restate_compound(seqs, k, count, thre, max_len)
    assert all(s[5] < MAXREC for s in want[1]) and sites                 # no site reaches the record cap
    assert [r for r in want[2] if not (r[2] == 1 and r[3] == 1)] == comp[1]
    assert [c[8] for c in want[0]] == [c[4] for c in comp[0]]             # the complex sites are the compound scan's
    return sites, want, comp


@pytest.mark.parametrize("i", range(4))
def test_explicit_sites_give_the_compound_scans_records(KT, i):
    what, k, thre, reads, text, seqs, count = explicit_workloads()[i]
    sites, want, comp = explicit_expectation(k, thre, seqs, count)
    t = KT(k, min_slots=1 << 16)
    if text is not None:
        t.count_text(text)
    else:
        t.count_bases(b"N".join(reads))
    rep = t.kmer_report(seqs, thre)
    assert compound_sites(rep.run_tuples(), k, 64) == sites
    gs = t.gap_search(seqs, thre, 64, sites)
    check_result(gs, want, what)
    assert gs.report is None
    cs = t.compound_scan(seqs, thre, 64)
    assert [r for r in gs.record_tuples() if not (r[2] == 1 and r[3] == 1)] == cs.record_tuples()
    assert [c[8] for c in gs.counts] == [c[4] for c in cs.counts]
    t.close()


def test_a_site_whose_flank_is_no_base_is_skipped(KT):
    k = 21
    truth, contig, plants = planted_fills(k, [5, 9], seed=5)
    (a0, n0, _, _), (a1, n1, _, _) = plants
    count = dict_counter(kmer_dict([truth] * 5, k))
    sites = [(0, a0, a0 + n0, 0), (0, a0 + n0 + k, a0 + n0 + k, 3), (0, a1 - 1, a1 + n1 - 1, 9), (1, k - 1, k - 1, 0)]      # the third: G starts with an N
    seqs = [contig, truth[:2 * k - 2]]
    want = restate_gap_search(seqs, k, count, 3, 50, sites)
    assert [s[4] for s in want[1]] == ["dead", "dead", "skipped", "dead"] and [s[9] for s in want[1]] == [0, 3, 9, 0] and [r[1] for r in want[2]] == [a0, a0 + n0 + k, k - 1]
    t = table_of(KT, k, [truth] * 5)
    check_result(t.gap_search(seqs, 3, 50, sites), want, "skipped")
    from jasper_amd.table import make_gap_sites
    check_result(t.gap_search(seqs, 3, 50, make_gap_sites(sites)), want, "from an array")
    assert t.gap_search(seqs, 3, 50, []).counts == [(0,) * 9] * 2
    t.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors(KT):
    import ctypes as C
    from jasper_amd import _lib
    from jasper_amd.table import make_gap_sites
    k = 21
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.gap_scan(s, 0)
        for bad in (4097, -1):
            with pytest.raises(_lib.JasperHipError, match="max_len"):
                t.gap_scan(s, 1, bad)
        with pytest.raises(_lib.JasperHipError, match="max_trim"):
            t.gap_scan(s, 1, 10, -1)
    for sites, msg in (([(0, k - 2, 30)], "out of bounds"), ([(0, 30, 200 - k + 2)], "out of bounds"), ([(0, 40, 39)], "a > q"), ([(1, 30, 30)], "no sequence"),
                       ([(0, 50, 50), (0, 30, 30)], "order"), ([(0, 30, 31), (0, 30, 32)], "order")):
        with pytest.raises(_lib.JasperHipError, match=msg):
            t.gap_search(seqs, 1, 10, sites)
    with pytest.raises(_lib.JasperHipError, match="thre"):
        t.gap_search(seqs, 0, 10, [(0, 30, 30)])
    with pytest.raises(_lib.JasperHipError, match="max_len"):
        t.gap_search(seqs, 1, 4097, [(0, 30, 30)])
    t1 = KT(1, min_slots=1 << 16)
    with pytest.raises(_lib.JasperHipError, match="k must"):
        t1.gap_scan(seqs, 1)
    t1.close()
    # the C-ABI: refused with no launch, and `out` stays NULL
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    lens = (C.c_int64 * 1)(200)
    res = C.c_void_p()
    arr = make_gap_sites([(0, 10, 30)])          # a < k - 1
    sp = C.c_void_p(arr.ctypes.data)
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 10, sp, 1, C.byref(res)) != 0 and not res
    arr = make_gap_sites([(0, 40, 39)])
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 10, C.c_void_p(arr.ctypes.data), 1, C.byref(res)) != 0 and not res
    ok = make_gap_sites([(0, 30, 34)])
    okp = C.c_void_p(ok.ctypes.data)
    assert L.jasper_gap_search(None, 1, cs, lens, 1, 10, okp, 1, C.byref(res)) != 0 and not res
    assert L.jasper_gap_search(t._h, 1, cs, lens, 0, 10, okp, 1, C.byref(res)) != 0 and not res
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 4097, okp, 1, C.byref(res)) != 0 and not res
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 10, None, 1, C.byref(res)) != 0 and not res
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 10, okp, 1, None) != 0
    assert L.jasper_gap_scan(t._h, 1, cs, (C.c_int64 * 1)(-5), 1, 10, 21, 0, C.byref(res)) != 0 and not res
    assert L.jasper_gap_scan(None, 1, cs, lens, 1, 10, 21, 0, C.byref(res)) != 0 and not res
    assert L.jasper_gap_scan(t._h, 1, cs, lens, 0, 10, 21, 0, C.byref(res)) != 0 and not res
    assert L.jasper_gap_scan(t._h, 1, cs, lens, 1, 4097, 21, 0, C.byref(res)) != 0 and not res
    assert L.jasper_gap_scan_device(t._h, 1, None, None, 1, 10, 21, 0, C.byref(res)) != 0 and not res
    assert L.jasper_gapscan_counts(None, 0, None) != 0 and L.jasper_gapscan_sites(None, None, None) != 0 and L.jasper_gapscan_records(None, None, None) != 0
    assert L.jasper_gapscan_bases(None, None, None) != 0 and L.jasper_gapscan_seconds(None, None, None, None) != 0 and L.jasper_gapscan_num_seqs(None) == 0
    assert L.jasper_gap_search(t._h, 1, cs, lens, 1, 10, okp, 1, C.byref(res)) == 0 and res
    c9 = (C.c_uint64 * 9)()
    assert L.jasper_gapscan_counts(res, 0, c9) == 0 and L.jasper_gapscan_counts(res, 1, c9) != 0 and L.jasper_gapscan_num_seqs(res) == 1 and c9[0] == 1
    assert L.jasper_report_num_seqs(L.jasper_gapscan_report(res)) == 0
    L.jasper_gapscan_free(res)
    count = dict_counter(kmer_dict([b"ACGT" * 100], k))
    check(t, seqs, 1, 64, k, True, restate_gaps(seqs, k, count, 1, 64, k, True), "a period of four")
    t.close()


def test_nothing_to_scan(KT):
    t = KT(21, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    gs = t.gap_scan([], 1)
    assert gs.counts == [] and len(gs.sites) == 0 and len(gs.records) == 0 and gs.bases == b"" and gs.lookups == 0
    gs = t.gap_scan(["", "ACG", "N" * 30, "ACGT" * 20], 1)
    assert gs.counts == [(0,) * 9, (0,) * 9, (1, 0, 0, 0, 0, 1, 0, 0, 0), (0,) * 9] and gs.site_tuples() == [(2, 20, 10, "gap", "edge", 0, 0, 0, 0, 0)]
    assert gs.lookups == 0 and gs.search_seconds == 0
    t.close()


# ---- the device entry, determinism, shards -----------------------------------------------------------------------------------------
def mixed_workload(k=37):
    """(reads, seqs, restatement at max_len 300 with long runs): planted fills, a dirty end, a long run, an edge gap, a ragged site, lower
    case, a tile seam, short and empty sequences"""
    truth, contig, plants = planted_fills(k, [0, 7, 40, 150, 260], seed=370)
    c = bytearray(contig)
    a2 = plants[2][0]
    c[a2 - 6] = ord("ACGT"["ACGT".index(chr(c[a2 - 6])) ^ 1])                     # a dirty end: trim_left 6
    c2 = bytearray(substitute(truth[:600], range(200, 290, 15)))                  # a long run
    c2[5] = ord("N")                                                              # an edge gap
    c2[400:402] = b"NN"
    c2[412] = ord("ACGT"["ACGT".index(chr(c2[412])) ^ 1])                         # ten bases after the gap: trim_right 11, with max_trim 6 it is ragged
    rng = np.random.default_rng(371)
    big = rand_bases(rng, TILE + 4 * k)
    cb = bytearray(big)
    cb[TILE - 3:TILE + 2] = b"NNNNN"                                              # an N run across the tile seam
    seqs = [bytes(c), bytes(c2), contig[:900].lower(), b"", contig[:k], bytes(cb)]
    reads = [truth] * 5 + [big] * 5
    want = restate_gaps(seqs, k, dict_counter(kmer_dict(reads, k)), 3, 300, 6, True)
    kinds = {(s[3], s[4]) for s in want[1]}
    assert {("gap", "dead"), ("run", "dead"), ("gap", "edge"), ("gap", "ragged")} <= kinds and sum(c[3] for c in want[0]) >= 8 and want[1][2][7] == 6
    return reads, seqs, want


def test_device_text_gives_what_host_text_gives_and_two_runs_are_equal(KT):
    import torch
    reads, seqs, want = mixed_workload()
    t = table_of(KT, 37, reads)
    gs = check(t, seqs, 3, 300, 6, True, want, "mixed")
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.gap_scan_device(d, offs, 3, 300, 6, True) == gs
    again = t.gap_scan(seqs, 3, 300, 6, True)
    assert again == gs and again.lookups == gs.lookups
    assert t.kmer_report(seqs, 3) == gs.report and t.compound_scan(seqs, 3, 64).report == gs.report and t.gap_scan(seqs, 3, 300, 6, True) == gs
    t.close()


@pytest.mark.parametrize("nshard", [2, 3])
def test_scan_through_owner_shards_equals_whole_table(KT, nshard):
    from test_gpu_shard import make_shards
    reads, seqs, want = mixed_workload()
    full = table_of(KT, 37, reads, 1 << 21)
    shards, _ = make_shards(KT, full, nshard, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    whole = check(full, seqs, 3, 300, 6, True, want, "whole")
    for t in shards:
        assert t.gap_scan(seqs, 3, 300, 6, True) == whole
    for t in shards + [full]:
        t.close()
