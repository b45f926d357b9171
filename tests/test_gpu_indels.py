"""GPU: the indel scan (KmerTable.indel_scan / indel_scan_device, jasper_indel_scan) against the restatement of its semantics in
test_indels_host.py, fed by Python dicts of canonical k-mer strings: the dict of a golden case's dump.txt.gz (printed by the real
`jellyfish dump -c`) or a dict of the reads' canonical k-mers.  Nothing expected here comes from the code under test.

The semantics are in test_indels_host.py's docstring (and include/jasper_hip.h).  The result also holds the variant scan of the same input
(IndelScan.variants); every workload here compares it with KmerTable.variant_scan, whose own tests are test_gpu_variants.py."""
import numpy as np
import pytest

import test_gpu_variants as tv
from golden_util import Case, case_names
from test_gpu_copies import TILE, as_bytes, dict_counter, is_wide, kmer_dict
from test_indels_host import ACGT, ERROR, HET, plant, rand_bases, restate

pytestmark = pytest.mark.gpu


def check(t, seqs, thre, max_len, want, what):
    """indel_scan against (counts, records) of the restatement, and its substitution half against variant_scan"""
    isc = t.indel_scan(seqs, thre, max_len)
    assert isc.counts == want[0], what
    got = isc.record_tuples()
    assert len(got) == len(want[1]), (what, len(got), len(want[1]))
    assert got == want[1], what
    assert all(bytes(r["pad"]) == bytes(7) for r in isc.records[:100])
    assert isc.variants == t.variant_scan(seqs, thre), what
    assert isc.check_seconds <= isc.seconds
    return isc


def kinds_and_types(recs):
    return {(r[2], r[7]) for r in recs}


ALL4 = {("ins", HET), ("ins", ERROR), ("del", HET), ("del", ERROR)}


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


def other(ch, step=1):
    """another base than the byte ch"""
    return ACGT[(ACGT.index(bytes([ch]).upper()) + step) % 4]


# ---- golden cases ------------------------------------------------------------------------------------------------------------------
# (insertions, deletions, candidates) from the restatement over the committed dumps at max_len 4, computed on the CPU.  The golden cases
# give both types but only kind `error` (their reads are one haplotype); het records of both types are test_constructed_edges' business.
ANCHORS = {"gaps_k25": (7, 13, 30), "gaps_k37_p4": (12, 9, 32), "homopolymer_k21": (3, 6, 10), "edges_k19": (1, 1, 8), "simple_k63": (3, 2, 9),
           "cluster_k25": (1, 0, 13)}


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    want = restate(seqs, c.k, count, c.thre, 4)
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    isc = check(t, seqs, c.thre, 4, want, name)
    t.close()
    n_ins, n_del = sum(r[2] == "ins" for r in want[1]), sum(r[2] == "del" for r in want[1])
    print(name, (n_ins, n_del, isc.variants.candidates))
    if name in ANCHORS:
        assert (n_ins, n_del, tv.restate(seqs, c.k, count, c.thre)[2]) == ANCHORS[name]
    assert isc.seconds > 0 and not isc.retried


def test_golden_anchors_hold_both_types():
    assert set(ANCHORS) <= set(case_names())
    assert any(i > 0 for i, _, _ in ANCHORS.values()) and any(d > 0 for _, d, _ in ANCHORS.values())


# ---- constructed edges -------------------------------------------------------------------------------------------------------------
def pair(s, events, reads):
    """the reads of a pair of haplotypes: 10 copies of s, 8 of s with the events"""
    reads += [s] * 10 + [plant(s, events)] * 8


def set_after(a, q, L):
    """make the deletion of a[q .. q+L-1] right-normalised at q: the byte after it differs from a[q]"""
    if a[q + L] == a[q]:
        a[q + L] = other(a[q])


def edges_workload():
    """-> (k, thre, reads, seqs, {sequence index: expected records at max_len 4})"""
    k, thre = 31, 5
    rng = np.random.default_rng(3107)
    n = 4 * TILE
    a = bytearray(rand_bases(rng, n))
    lens = [1, 2, 4, 5]
    het, err, want0 = [], [], []
    for i, L in enumerate(lens):
        for events, q0, rmin, amin, kind in ((het, 1000, 10, 8, HET), (err, 5000, 0, 18, ERROR)):
            q = q0 + 300 * i                                        # an insertion of x^L before q
            x = other(a[q], 1 + i % 3)
            events.append((q, "ins", L, x))
            if L <= 4:
                want0.append((0, q, "ins", L, chr(x), rmin, amin, kind))
            q = q0 + 1500 + 300 * i                                 # a deletion of L bytes at q
            set_after(a, q, L)
            events.append((q, "del", L, None))
            if L <= 4:
                want0.append((0, q, "del", L, chr(a[q + L]), rmin, amin, kind))
    # a homopolymer one longer in the second haplotype, reported at the first window end of tile 1 ...
    p1 = TILE + k - 1
    a[p1 - 4:p1 + 1] = b"TTTTG"
    het.append((p1, "ins", 1, ord("T")))
    want0.append((0, p1, "ins", 1, "T", 10, 8, HET))
    # ... and one a base shorter, reported at the last window end of tile 2
    p2 = 3 * TILE + k - 2
    a[p2 - 3:p2 + 2] = b"TTTTC"
    het.append((p2, "del", 1, None))
    want0.append((0, p2, "del", 1, "C", 10, 8, HET))
    a = bytes(a)
    reads = [plant(a, sorted(err))] * 10 + [plant(a, sorted(err + het))] * 8
    asm = a[:1200] + a[1200:2900].lower() + a[2900:]                # lower case over a het insertion and a het deletion
    seqs, want = [asm], {0: sorted(want0, key=lambda r: r[1])}

    def short(s, events, expect):
        pair(s, events, reads)
        seqs.append(s)
        want[len(seqs) - 1] = [(len(seqs) - 1,) + e for e in expect]

    # an insertion at p = n - k + 1 is evaluated, at n - k + 2 it is not
    for d, found in ((1, True), (2, False)):
        s = rand_bases(rng, 300)
        p = 300 - k + d
        x = other(s[p])
        short(s, [(p, "ins", 1, x)], [(p, "ins", 1, chr(x), 10, 8, HET)] if found else [])
    # a deletion whose context ends on the last byte (p + L + k - 2 = n - 1), and one byte short of it
    for d, found in ((1, True), (2, False)):
        s = bytearray(rand_bases(rng, 300))
        p = 300 - 2 - k + d
        set_after(s, p, 2)
        s = bytes(s)
        short(s, [(p, "del", 2, None)], [(p, "del", 2, chr(s[p + 2]), 10, 8, HET)] if found else [])
    # an N inside the deleted bytes, on the first and on the last byte of the context, and just outside it on either side
    b = bytearray(rand_bases(rng, 400))
    set_after(b, 200, 3)
    b = bytes(b)
    pair(b, [(200, "del", 3, None)], reads)
    for at, found in ((201, False), (200 - k + 1, False), (200 + 3 + k - 2, False), (200 + 3 + k - 1, True), (200 - k, True)):
        seqs.append(b[:at] + b"N" + b[at + 1:])
        want[len(seqs) - 1] = [(len(seqs) - 1, 200, "del", 3, chr(b[203]), 10, 8, HET)] if found else []
    # sequences of 2k - 2, 2k - 3 and 2k - 1 bytes around an insertion at k - 1, and an empty one
    c = rand_bases(rng, 2 * k - 1)
    x = other(c[k - 1])
    pair(c, [(k - 1, "ins", 2, x)], reads)
    for s, found in ((c[:2 * k - 2], True), (c[1:2 * k - 2], False), (c, True), (b"", False)):
        seqs.append(s)
        want[len(seqs) - 1] = [(len(seqs) - 1, k - 1, "ins", 2, chr(x), 10, 8, HET)] if found else []
    return k, thre, reads, seqs, want


def test_constructed_edges(KT):
    k, thre, reads, seqs, want_by_seq = edges_workload()
    assert [len(s) for s in seqs[-4:]] == [2 * k - 2, 2 * k - 3, 2 * k - 1, 0] and len(seqs[0]) == 4 * TILE and len(seqs) == 14
    count = dict_counter(kmer_dict(reads, k))
    want = restate(seqs, k, count, thre, 4)
    counts, recs = want
    for si in range(len(seqs)):
        assert [r for r in recs if r[0] == si] == want_by_seq[si], si
    assert counts[0] == (4, 3, 4, 3) and kinds_and_types(recs) == ALL4
    assert {r[3] for r in recs if r[0] == 0} == {1, 2, 4}
    assert {TILE + k - 1, 3 * TILE + k - 2} <= {r[1] for r in recs if r[0] == 0}
    # with max_len 5 the planted events of length 5 appear as well: two insertions and two deletions more
    want5 = restate(seqs[:1], k, count, thre, 5)
    assert want5[0] == [(5, 4, 5, 4)] and {r[3] for r in want5[1]} == {1, 2, 4, 5}
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    isc = check(t, seqs, thre, 4, want, "edges")
    check(t, seqs[:1], thre, 5, want5, "edges, max_len 5")
    print(isc.counts, isc.variants.candidates, isc.lookups)
    assert isc.lookups > 0 and not isc.retried
    t.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
FUZZ_KS = [2, 3, 5, 16, 17, 31, 32, 33, 37, 63, 64]


def random_events(rng, g, lo, hi, step):
    """isolated events on g: alternately a same-base insertion and a deletion, lengths 1 .. 17 in turn"""
    ev = []
    for i, q0 in enumerate(range(lo, hi, step)):
        q = q0 + int(rng.integers(0, step // 4))
        L = (1, 2, 4, 16, 3, 17, 5, 9)[(i // 2) % 8]
        if q + L + 1 >= len(g):
            break
        ev.append((q, "ins", L, ACGT[int(rng.integers(0, 4))]) if i % 2 == 0 else (q, "del", L, None))
    return ev


def fuzz_workload(k):
    """a genome of 3000 bases (300 for k <= 5, where nearly every hypothesis is a record); reads: four haplotypes with substitutions and
    planted indels of their own at 3, 2, 1 and 1 copies, so that every threshold 1..4 separates some alleles from others; the scanned
    sequences: the genome with indels and substitutions of its own, N runs, other non-base bytes and lower case, and pieces of it"""
    rng = np.random.default_rng(7300 + k)
    G = 3000 if k > 5 else 300
    step = 3 * k + 40
    g = rand_bases(rng, G)
    reads = []
    for i, copies in enumerate((3, 2, 1, 1)):
        h = tv.substituted(g, sorted(rng.choice(G, G // 250 + 1, replace=False).tolist()), int(rng.integers(1, 4)))
        reads += [plant(h, random_events(rng, h, 50 + i * step // 4, G - 50, step))] * copies
    a = plant(g, random_events(rng, g, 50 + step // 2, G - 50, 2 * step))
    a = bytearray(tv.substituted(a, sorted(rng.choice(len(a), G // 300 + 1, replace=False).tolist()), 2))
    for p in rng.integers(0, len(a) - 40, 2).tolist():
        a[p:p + int(rng.integers(1, 30))] = b"N"
    lo = int(rng.integers(0, len(a) // 2))
    a[lo:lo + len(a) // 3] = bytes(a[lo:lo + len(a) // 3]).lower()
    for p, ch in zip(rng.integers(0, len(a), 4).tolist(), b"nR-*"):
        a[p] = ch
    a = bytes(a)
    seqs = [a, b"", g[100:100 + 2 * k - 3], g[120:120 + 2 * k - 2], g[140:140 + 2 * k - 1].lower(), g[:min(G, 1000)]]
    for _ in range(6):
        p = int(rng.integers(0, len(a) - 200))
        seqs.append(a[p:p + int(rng.integers(0, 200))])
    return reads, seqs


@pytest.mark.parametrize("k", FUZZ_KS)
def test_fuzz_against_dicts(KT, k):
    import torch
    reads, seqs = fuzz_workload(k)
    assert max(len(s) for s in seqs) <= 10_000
    count = dict_counter(kmer_dict(reads, k))
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    if k >= 37:
        assert is_wide(t)
    if k <= 32:
        assert not is_wide(t)
    seen = set()
    for thre in (1, 2, 3, 4):
        for max_len in (1, 4, 16):
            want = restate(seqs, k, count, thre, max_len)
            isc = check(t, seqs, thre, max_len, want, (k, thre, max_len))
            print(k, thre, max_len, [sum(c[i] for c in want[0]) for i in range(4)], isc.variants.candidates, isc.lookups)
            seen |= kinds_and_types(want[1])
            if max_len == 16 and thre == 1:
                assert max([r[3] for r in want[1]], default=0) > 4
    if k >= 16:
        assert seen == ALL4
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.indel_scan_device(d, offs, 2, 16) == t.indel_scan(seqs, 2, 16)      # host text and device text give the same object
    t.close()


# ---- table shapes ------------------------------------------------------------------------------------------------------------------
def small_workload(seed, k, G=20_000):
    """two haplotypes that differ by an indel every 211 bases (reads: 6 and 5 copies) and an assembly with indels of its own"""
    rng = np.random.default_rng(seed)
    h1 = rand_bases(rng, G)
    reads = [h1] * 6 + [plant(h1, random_events(rng, h1, 97, G - 97, 211))] * 5
    asm = plant(h1, random_events(rng, h1, 1000, G - 1000, 1777))
    seqs = [asm, asm[2000:9000].lower(), b"", asm[:2 * k - 3], asm[3000:3000 + TILE + 3 * k], asm[500:900] + b"N" + asm[901:1400]]
    return reads, seqs


_small = {}


def small_expected(seed, k, thre, max_len):
    """(reads, seqs, restatement), computed once per workload"""
    key = (seed, k, thre, max_len)
    if key not in _small:
        reads, seqs = small_workload(seed, k)
        _small[key] = reads, seqs, restate(seqs, k, dict_counter(kmer_dict(reads, k)), thre, max_len)
    return _small[key]


@pytest.mark.parametrize("slots,wide", [(1 << 16, True), (1 << 22, False)])
def test_narrow_against_wide(KT, slots, wide):
    """k = 37 is wide below 2^21 slots and narrow from there on: the same workload in tables of two sizes, the same result"""
    k = 37
    reads, seqs, want = small_expected(77, k, 3, 4)
    assert kinds_and_types(want[1]) == ALL4 and len(want[1]) > 50
    t = KT(k, min_slots=slots)
    t.count_bases(b"N".join(reads))
    assert is_wide(t) == wide
    check(t, seqs, 3, 4, want, slots)
    t.close()


@pytest.mark.parametrize("nshard", [2, 3])
def test_scan_through_owner_shards_equals_whole_table(KT, nshard):
    from test_gpu_shard import make_shards
    k = 37
    reads, seqs, want = small_expected(77, k, 3, 4)
    full = KT(k, min_slots=1 << 21)
    full.count_bases(b"N".join(reads))
    shards, _ = make_shards(KT, full, nshard, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    whole = check(full, seqs, 3, 4, want, "whole")
    for t in shards:
        assert t.indel_scan(seqs, 3, 4) == whole
    for t in shards + [full]:
        t.close()


def test_more_records_than_candidates_and_than_the_first_list(KT):
    """k = 4, a random 1000-base sequence counted as its own reads, thre 1, max_len 16: nearly all 136 canonical 4-mers are present, so
    nearly every hypothesis that is evaluated is a record -- up to 48 insertions per position and a deletion for most lengths: far more
    records than the three candidates per position, and than the first list (candidates + 4096)"""
    k = 4
    s = rand_bases(np.random.default_rng(404), 1000)
    rd = kmer_dict([s], k)
    assert len(rd) >= 130
    count = dict_counter(rd)
    want = restate([s], k, count, 1, 16)
    ncand = tv.restate([s], k, count, 1)[2]
    assert 2900 < ncand <= 3 * (1000 - k + 1) and len(want[1]) > 5 * (ncand + 4096)
    assert want[0][0][0] > 40_000 and want[0][0][2] > 10_000 and want[0][0][1] == 0 and want[0][0][3] == 0
    t = KT(k, min_slots=1 << 16)
    t.count_bases(s)
    isc = check(t, [s], 1, 16, want, "dense")
    assert isc.retried and isc.variants.candidates == ncand
    isc = t.indel_scan([s], max(rd.values()) + 1, 16)
    assert isc.counts == [(0, 0, 0, 0)] and len(isc.records) == 0 and not isc.retried and isc.variants.candidates == 0
    t.close()


def test_ten_calls_and_interleaved_scans_keep_their_results_and_leave_the_table_alone(KT):
    from test_gpu_copies import asm_table, histo_of, peak_rule
    k = 37
    reads, seqs, want = small_expected(77, k, 3, 4)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    a = asm_table(KT, k, seqs)
    before = t.info(), list(t.histogram())
    first = check(t, seqs, 3, 4, want, "first")
    assert len(first.records) > 50
    peak = peak_rule(histo_of(kmer_dict(reads, k)), 3)
    krep, crep, vs = t.kmer_report(seqs, 3), t.copy_report(a, seqs, 3, peak), t.variant_scan(seqs, 3)
    for _ in range(9):
        assert t.indel_scan(seqs, 3, 4) == first
    # a report, a copy scan, a variant scan and an indel scan of one table keep their own buffers
    assert t.kmer_report(seqs, 3) == krep
    assert t.indel_scan(seqs, 3, 4) == first
    assert t.copy_report(a, seqs, 3, peak) == crep
    assert t.indel_scan(seqs[:2], 3, 4).counts == first.counts[:2]
    assert t.variant_scan(seqs, 3) == vs
    assert t.indel_scan(seqs, 3, 4) == first
    assert t.kmer_report(seqs, 3) == krep and t.copy_report(a, seqs, 3, peak) == crep and t.variant_scan(seqs, 3) == vs
    assert (t.info(), list(t.histogram())) == before
    t.close()
    a.close()


def test_an_empty_table_gives_no_record(KT):
    k = 31
    _, seqs = small_workload(10, k)
    zeros = [(0, 0, 0, 0)] * len(seqs)
    empty = KT(k, min_slots=1 << 16)                  # never counted into: logically empty, its memory was never written
    isc = empty.indel_scan(seqs, 1, 16)
    assert isc.counts == zeros and len(isc.records) == 0 and isc.variants == empty.variant_scan(seqs, 1) and isc.variants.candidates == 0
    empty.count_bases(seqs[0])
    empty.clear()                                     # cleared: logically empty again
    isc = empty.indel_scan(seqs, 1, 16)
    assert isc.counts == zeros and len(isc.records) == 0 and isc.variants.candidates == 0
    assert empty.indel_scan([], 1).counts == [] and empty.indel_scan(["", "ACG"], 1).counts == [(0, 0, 0, 0)] * 2
    empty.close()


def test_bad_arguments_are_errors(KT):
    import ctypes as C
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):                                      # (also with nothing to scan)
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.indel_scan(s, 0)
        for bad in (0, 17, -1):
            with pytest.raises(_lib.JasperHipError, match="max_len"):
                t.indel_scan(s, 1, bad)
    t1 = KT(1, min_slots=1 << 16)
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="k must"):
            t1.indel_scan(s, 1)
    t1.close()
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    res = C.c_void_p()
    assert L.jasper_indel_scan(t._h, 1, cs, (C.c_int64 * 1)(-5), 1, 4, C.byref(res)) != 0 and not res           # a negative length
    assert L.jasper_indel_scan(t._h, 1, cs, (C.c_int64 * 1)(200), 1, 4, None) != 0                              # a null output
    assert L.jasper_indel_scan(None, 1, cs, (C.c_int64 * 1)(200), 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indel_scan_device(t._h, 1, None, (C.c_int64 * 2)(10, 5), 1, 4, C.byref(res)) != 0 and not res   # offsets that decrease
    assert L.jasper_indel_scan_device(t._h, 1, None, None, 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indelscan_counts(None, 0, None) != 0 and L.jasper_indelscan_records(None, None, None) != 0 and not L.jasper_indelscan_variants(None)
    check(t, seqs, 1, 16, restate(seqs, 31, dict_counter(kmer_dict([b"ACGT" * 100], 31)), 1, 16), "a period of four")
    t.close()
