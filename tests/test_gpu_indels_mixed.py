"""GPU: the mixed half of the indel scan (KmerTable.indel_scan(.., mixed=True), jasper_indel_scan_mixed) against the restatement of its
semantics in test_indels_mixed_host.py, fed by Python dicts of canonical k-mer strings.  Nothing expected here comes from the code under
test.  Every workload also states that the old half is unchanged (scan(mixed=True) == scan(mixed=False), which compares counters,
records and the substitution half) and that the substitution half is variant_scan's."""
import itertools

import numpy as np
import pytest

import test_gpu_indels as ti
from golden_util import Case, case_names
from test_gpu_copies import TILE, dict_counter, is_wide, kmer_dict
from test_indels_host import ACGT, ERROR, HET, rand_bases, restate
from test_indels_mixed_host import FRONT, MIXED_ANCHORS, left_most, plant_strings, random_string, restate_mixed, right_most

pytestmark = pytest.mark.gpu


def check(t, seqs, thre, max_len, want, what):
    """indel_scan(mixed=True) against (counts, records) of the restatement; its other half against the scan without `mixed`"""
    isc = t.indel_scan(seqs, thre, max_len, mixed=True)
    m = isc.mixed
    assert m is not None and m.counts == want[0], what
    got = m.record_tuples()
    assert len(got) == len(want[1]), (what, len(got), len(want[1]))
    assert got == want[1], what
    assert all(bytes(r["pad"]) == bytes(5) for r in m.records[:100])
    plain = t.indel_scan(seqs, thre, max_len)
    assert plain.mixed is None and isc == plain, what
    assert isc.variants == t.variant_scan(seqs, thre), what
    assert m.seconds <= isc.seconds
    return isc


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
    want = restate_mixed(seqs, c.k, count, c.thre, 4)
    assert len(want[1]) == MIXED_ANCHORS.get(name, 0)
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    isc = check(t, seqs, c.thre, 4, want, name)
    t.close()
    assert not isc.mixed.retried and (isc.mixed.lookups > 0) == (isc.variants.candidates > 0)


# ---- both sides of one pair --------------------------------------------------------------------------------------------------------
PAIR_LENS = (1, 2, 3, 4, 5, 8, 16)


def pair_workload(seed=911, n=4000):
    """h1, and h2 = h1 with an insertion of a random string and a deletion of each length of PAIR_LENS, 250 bytes apart; reads: 6 copies
    of h1 and 5 of h2 -> (h1, h2, reads, events)"""
    rng = np.random.default_rng(seed)
    h1 = rand_bases(rng, n)
    events = []
    for i in range(2 * len(PAIR_LENS)):
        q = 300 + 250 * i + int(rng.integers(0, 20))
        L = PAIR_LENS[i // 2]
        events.append((q, "ins", random_string(rng, L)) if i % 2 == 0 else (q, "del", L))
    return h1, plant_strings(h1, events), events


def insertions_of(isc):
    """every insertion of a result, same-base and mixed: {(pos, y)}"""
    out = {(r[1], r[4] * r[3]) for r in isc.record_tuples() if r[2] == "ins"}
    return out | {(r[1], r[3]) for r in isc.mixed.record_tuples()}


def deletions_of(isc):
    return {(r[1], r[3]) for r in isc.record_tuples() if r[2] == "del"}


def left_most_del(s, q, L):
    while q > 1 and s[q - 1] == s[q + L - 1]:
        q -= 1
    return q


@pytest.mark.parametrize("k", [31, 64])
def test_both_sides_of_one_pair(KT, k):
    h1, h2, events = pair_workload()
    reads = [h1] * 6 + [h2] * 5
    count = dict_counter(kmer_dict(reads, k))
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    s1 = check(t, [h1], 3, 16, restate_mixed([h1], k, count, 3, 16), "h1")
    s2 = check(t, [h2], 3, 16, restate_mixed([h2], k, count, 3, 16), "h2")
    t.close()
    ins1, ins2, del1, del2 = insertions_of(s1), insertions_of(s2), deletions_of(s1), deletions_of(s2)
    assert len(ins1) == len(ins2) == len(del1) == len(del2) == len(PAIR_LENS)
    shift = 0
    for q, typ, v in events:
        if typ == "ins":                                  # h1 sees an insertion of v, h2 a deletion of len(v) bytes
            here, there, L, y = h1, h2, len(v), v
            pi, pd, ins, dels, d = q, q + shift, ins1, del2, shift
            shift += L
        else:                                             # h2 sees an insertion of the bytes h1 holds, h1 a deletion
            here, there, L, y = h2, h1, v, h1[q:q + v]
            pi, pd, ins, dels, d = q + shift, q, ins2, del1, -shift
            shift -= L
        rp, ry = right_most(here, pi, y)
        assert (rp, ry.decode()) in ins, (q, typ)
        while there[pd + L] == there[pd]:                 # the deletion at its right-most position
            pd += 1
        assert (pd, L) in dels, (q, typ)
        # after left alignment both views name the same anchor byte (d = the offset of `there` against `here`)
        assert left_most(here, rp, ry)[0] + d == left_most_del(there, pd, L), (q, typ)
    assert {len(y) for _, y in ins1} == set(PAIR_LENS) and s1.mixed.counts[0][2] == 0 and s2.mixed.counts[0][2] == 0
    assert all(r[6] == HET for r in s1.mixed.record_tuples() + s2.mixed.record_tuples())


# ---- constructed edges -------------------------------------------------------------------------------------------------------------
def not_starting(y, ch):
    """the string y with another first base if it starts with the byte ch"""
    return (bytes([ti.other(ch, 1 if ti.other(ch) != y[1] else 2)]) + y[1:]) if y[0] == ch else y


def edges_workload():
    """-> (k, thre, reads, seqs, {sequence index: expected records at max_len 4})"""
    k, thre = 31, 5
    rng = np.random.default_rng(4242)
    n = 4 * TILE
    a = bytearray(rand_bases(rng, n))
    het, err, want0 = [], [], []
    strings = [b"CA", b"GAT", b"TGCA", b"ACGTC"]
    for i, y0 in enumerate(strings):
        for events, q0, rmin, amin, kind in ((het, 1000, 10, 8, HET), (err, 5000, 0, 18, ERROR)):
            q = q0 + 300 * i
            y = not_starting(y0, a[q])
            events.append((q, "ins", y))
            if len(y) <= 4:
                want0.append((0, q, len(y), y.decode(), rmin, amin, kind))
    # one reported at the first window end of tile 1 and one at the last of tile 2
    p1 = TILE + k - 1
    a[p1] = ord("G")
    het.append((p1, "ins", b"TC"))
    want0.append((0, p1, 2, "TC", 10, 8, HET))
    p2 = 3 * TILE + k - 2
    a[p2] = ord("A")
    het.append((p2, "ins", b"CGT"))
    want0.append((0, p2, 3, "CGT", 10, 8, HET))
    # a planted string whose first base is s[q]: AGT before AGC.. is GTA before the G and TAG before the C, the right-most position
    q = 2400
    a[q:q + 3] = b"AGC"
    het.append((q, "ins", b"AGT"))
    want0.append((0, q + 2, 3, "TAG", 10, 8, HET))
    # a tandem copy: ..ACAC|G + AC
    q = 2800
    a[q - 5:q + 1] = b"TACACG"
    het.append((q, "ins", b"AC"))
    want0.append((0, q, 2, "AC", 10, 8, HET))
    a = bytes(a)
    reads = [plant_strings(a, sorted(err))] * 10 + [plant_strings(a, sorted(err + het))] * 8
    asm = a[:1200] + a[1200:2900].lower() + a[2900:]                # lower case over het insertions
    seqs, want = [asm], {0: sorted(want0, key=lambda r: r[1])}

    def short(s, events, expect):
        reads.extend([s] * 10 + [plant_strings(s, events)] * 8)
        seqs.append(s)
        want[len(seqs) - 1] = [(len(seqs) - 1,) + e for e in expect]

    # an insertion at p = n - k + 1 is evaluated, at n - k + 2 it is not
    for d, found in ((1, True), (2, False)):
        s = rand_bases(rng, 300)
        p = 300 - k + d
        y = not_starting(b"GC", s[p])
        short(s, [(p, "ins", y)], [(p, 2, y.decode(), 10, 8, HET)] if found else [])
    # an N on the first and on the last byte of the context, and just outside it on either side
    b = rand_bases(rng, 400)
    y = not_starting(b"TGA", b[200])
    reads.extend([b] * 10 + [plant_strings(b, [(200, "ins", y)])] * 8)
    for at, found in ((200 - k + 1, False), (200 + k - 2, False), (200 + k - 1, True), (200 - k, True)):
        seqs.append(b[:at] + b"N" + b[at + 1:])
        want[len(seqs) - 1] = [(len(seqs) - 1, 200, 3, y.decode(), 10, 8, HET)] if found else []
    # sequences of 2k - 2, 2k - 3 and 2k - 1 bytes around an insertion at k - 1, and an empty one
    c = rand_bases(rng, 2 * k - 1)
    y = not_starting(b"CT", c[k - 1])
    reads.extend([c] * 10 + [plant_strings(c, [(k - 1, "ins", y)])] * 8)
    for s, found in ((c[:2 * k - 2], True), (c[1:2 * k - 2], False), (c, True), (b"", False)):
        seqs.append(s)
        want[len(seqs) - 1] = [(len(seqs) - 1, k - 1, 2, y.decode(), 10, 8, HET)] if found else []
    return k, thre, reads, seqs, want


def test_constructed_edges(KT):
    k, thre, reads, seqs, want_by_seq = edges_workload()
    assert [len(s) for s in seqs[-4:]] == [2 * k - 2, 2 * k - 3, 2 * k - 1, 0] and len(seqs[0]) == 4 * TILE and len(seqs) == 11
    count = dict_counter(kmer_dict(reads, k))
    want = restate_mixed(seqs, k, count, thre, 4)
    counts, recs = want
    for si in range(len(seqs)):
        assert [r for r in recs if r[0] == si] == want_by_seq[si], si
    assert counts[0] == (7, 3, 0) and {r[2] for r in recs if r[0] == 0} == {2, 3, 4}
    assert {TILE + k - 1, 3 * TILE + k - 2} <= {r[1] for r in recs if r[0] == 0}
    # with max_len 5 the planted strings of length 5 appear as well
    want5 = restate_mixed(seqs[:1], k, count, thre, 5)
    assert want5[0] == [(8, 4, 0)] and {r[2] for r in want5[1]} == {2, 3, 4, 5}
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    isc = check(t, seqs, thre, 4, want, "edges")
    check(t, seqs[:1], thre, 5, want5, "edges, max_len 5")
    print(isc.mixed.counts, isc.variants.candidates, isc.mixed.lookups)
    assert isc.mixed.lookups > 0 and not isc.mixed.retried
    t.close()


# ---- the cap -----------------------------------------------------------------------------------------------------------------------
def test_the_cap(KT):
    """k = 5 and thre 1 on random reads: most 5-mers are present, so the frontier grows until it is cut.  Levels of exactly 64 prefixes
    are searched, levels of 65 are not; at max_len 8 and 16 the level passes k, where a window holds nothing of F any more."""
    rng = np.random.default_rng(5)
    reads = [rand_bases(rng, 330)]
    asm = rand_bases(rng, 300)
    k = 5
    count = dict_counter(kmer_dict(reads, k))
    st = {}
    want = restate_mixed([asm], k, count, 1, 6, st)
    assert (st["candidates"], st["complex"], st["candidates"] - st["complex"]) == (420, 271, 149)
    assert st["levels"].count(FRONT) == 8 and st["levels"].count(FRONT + 1) == 5 and want[0][0][2] == 271
    t = KT(k, min_slots=1 << 16)
    t.count_bases(reads[0])
    check(t, [asm], 1, 6, want, "cap")
    for max_len in (4, 8, 16):
        st = {}
        want = restate_mixed([asm], k, count, 1, max_len, st)
        assert (st["complex"] == 0) == (max_len == 4) and len(want[1]) > 1000
        if max_len > k:
            assert max(r[2] for r in want[1]) > k
        check(t, [asm], 1, max_len, want, ("cap", max_len))
    t.close()


def test_more_records_than_the_first_list(KT):
    """k = 4 with every 4-mer in the reads: every string is solid, so every candidate gives the 3 + 15 + 63 strings of lengths 2, 3 and 4
    that are not x^t, and 256 prefixes of length 5: complex.  Far more records than the first list (candidates + 4096) holds."""
    k = 4
    reads = [bytes(w) for w in itertools.product(ACGT, repeat=k)]
    s = rand_bases(np.random.default_rng(404), 300)
    count = dict_counter(kmer_dict(reads, k))
    ncand = 3 * (300 - 2 * k + 3)                             # three alternatives at every p in k-1 .. n-k+1
    want = restate_mixed([s], k, count, 1, 6)
    assert want[0] == [(0, 81 * ncand, ncand)] or want[0] == [(81 * ncand, 0, ncand)]
    assert len(want[1]) == 81 * ncand > 5 * (3 * 300 + 4096)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    isc = check(t, [s], 1, 6, want, "dense")
    assert isc.mixed.retried and isc.mixed.counts[0][2] == ncand
    assert (isc.counts, isc.record_tuples()) == restate([s], k, count, 1, 6)      # the same-base list is not disturbed
    t.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ti.FUZZ_KS)
def test_fuzz_against_dicts(KT, k):
    """test_gpu_indels.fuzz_workload (same-base insertions, deletions, substitutions, N runs, lower case, pieces) and two more reads: a
    clean piece of the genome, which is also scanned, with insertions of random strings"""
    import torch
    reads, seqs = ti.fuzz_workload(k)
    rng = np.random.default_rng(9100 + k)
    g = seqs[5]
    step = max(len(g) // 12, 8)
    reads = reads + [plant_strings(g, [(q, "ins", random_string(rng, (2, 3, 5, 16, 4, 9)[i % 6])) for i, q in enumerate(range(step, len(g) - step, step))])] * 2
    count = dict_counter(kmer_dict(reads, k))
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    total = 0
    for thre, max_len in itertools.product((1, 2, 3), (1, 4, 16)) if k > 5 else ((1, 1), (1, 3), (1, 6), (2, 6), (3, 3)) if k == 5 else ((1, 1), (1, 3), (2, 2), (3, 3)):
        if True:                                              # (a small k makes nearly every string a record, 4^L of them: fewer rounds)
            want = restate_mixed(seqs, k, count, thre, max_len)
            isc = check(t, seqs, thre, max_len, want, (k, thre, max_len))
            print(k, thre, max_len, [sum(c[i] for c in want[0]) for i in range(3)], isc.variants.candidates, isc.mixed.lookups)
            assert max_len > 1 or not want[1]                # (a string of one base is a same-base string)
            total += len(want[1])
    assert total > 0
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    a, b = t.indel_scan_device(d, offs, 2, 6, mixed=True), t.indel_scan(seqs, 2, 6, mixed=True)
    assert a == b and a.mixed == b.mixed                      # host text and device text give the same object
    t.close()


# ---- table shapes ------------------------------------------------------------------------------------------------------------------
_small = {}


def small_workload(seed, k, G=8000):
    """two haplotypes that differ by an insertion of a random string or a deletion every 211 bases (reads: 6 and 5 copies) and an
    assembly, the first haplotype with such events of its own: its deletions are the reads' insertions of kind error"""
    rng = np.random.default_rng(seed)

    def events(lo, hi, step):
        ev = []
        for i, q in enumerate(range(lo, hi, step)):
            L = (2, 3, 1, 16, 5, 4, 9, 7)[i % 8]
            ev.append((q, "ins", random_string(rng, L)) if i % 2 == 0 else (q, "del", L))
        return ev

    h1 = rand_bases(rng, G)
    reads = [h1] * 6 + [plant_strings(h1, events(97, G - 97, 211))] * 5
    asm = plant_strings(h1, events(500, G - 500, 977))
    return reads, [asm, asm[2000:5000].lower(), b"", asm[:2 * k - 3], asm[3000:3000 + TILE + 3 * k], asm[500:900] + b"N" + asm[901:1400]]


def small_expected(k=37, thre=3, max_len=16):
    """(reads, seqs, restatement), computed once"""
    key = (k, thre, max_len)
    if key not in _small:
        reads, seqs = small_workload(77, k)
        _small[key] = reads, seqs, restate_mixed(seqs, k, dict_counter(kmer_dict(reads, k)), thre, max_len)
    return _small[key]


@pytest.mark.parametrize("slots,wide", [(1 << 16, True), (1 << 22, False)])
def test_narrow_against_wide(KT, slots, wide):
    reads, seqs, want = small_expected()
    assert len(want[1]) > 20 and {r[6] for r in want[1]} == {HET, ERROR}
    t = KT(37, min_slots=slots)
    t.count_bases(b"N".join(reads))
    assert is_wide(t) == wide
    check(t, seqs, 3, 16, want, slots)
    t.close()


@pytest.mark.parametrize("nshard", [2, 3])
def test_scan_through_owner_shards_equals_whole_table(KT, nshard):
    from test_gpu_shard import make_shards
    reads, seqs, want = small_expected()
    full = KT(37, min_slots=1 << 21)
    full.count_bases(b"N".join(reads))
    shards, _ = make_shards(KT, full, nshard, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    whole = check(full, seqs, 3, 16, want, "whole")
    for t in shards:
        got = t.indel_scan(seqs, 3, 16, mixed=True)
        assert got == whole and got.mixed == whole.mixed
    for t in shards + [full]:
        t.close()


def test_ten_calls_and_interleaved_scans_keep_their_results_and_leave_the_table_alone(KT):
    from test_gpu_copies import asm_table, histo_of, peak_rule
    k = 37
    reads, seqs, want = small_expected()
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    a = asm_table(KT, k, seqs)
    before = t.info(), list(t.histogram())
    first = check(t, seqs, 3, 16, want, "first")
    peak = peak_rule(histo_of(kmer_dict(reads, k)), 3)
    krep, crep, vs, plain = t.kmer_report(seqs, 3), t.copy_report(a, seqs, 3, peak), t.variant_scan(seqs, 3), t.indel_scan(seqs, 3, 16)

    def again():
        got = t.indel_scan(seqs, 3, 16, mixed=True)
        assert got == first and got.mixed == first.mixed and got.mixed.lookups == first.mixed.lookups

    for _ in range(5):
        again()
    assert t.kmer_report(seqs, 3) == krep
    again()
    assert t.copy_report(a, seqs, 3, peak) == crep
    again()
    assert t.variant_scan(seqs, 3) == vs
    again()
    assert t.indel_scan(seqs, 3, 16) == plain and t.indel_scan(seqs[:2], 3, 4, mixed=True).mixed.counts == restate_mixed(seqs[:2], k, dict_counter(kmer_dict(reads, k)), 3, 4)[0]
    again()
    assert t.kmer_report(seqs, 3) == krep and t.copy_report(a, seqs, 3, peak) == crep and t.variant_scan(seqs, 3) == vs and t.indel_scan(seqs, 3, 16) == plain
    assert (t.info(), list(t.histogram())) == before
    t.close()
    a.close()


def test_an_empty_table_gives_nothing(KT):
    k = 31
    _, seqs = small_workload(10, k)
    empty = KT(k, min_slots=1 << 16)
    for _ in range(2):
        isc = empty.indel_scan(seqs, 1, 16, mixed=True)
        assert isc.mixed.counts == [(0, 0, 0)] * len(seqs) and len(isc.mixed.records) == 0 and isc.mixed.lookups == 0 and not isc.mixed.retried
        assert isc == empty.indel_scan(seqs, 1, 16)
        empty.count_bases(seqs[0])
        empty.clear()
    assert empty.indel_scan([], 1, mixed=True).mixed.counts == [] and empty.indel_scan(["", "ACG"], 1, mixed=True).mixed.counts == [(0, 0, 0)] * 2
    empty.close()


def test_bad_arguments_are_errors_and_a_plain_result_has_an_empty_mixed_half(KT):
    import ctypes as C
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.indel_scan(s, 0, mixed=True)
        for bad in (0, 17, -1):
            with pytest.raises(_lib.JasperHipError, match="max_len"):
                t.indel_scan(s, 1, bad, mixed=True)
    t1 = KT(1, min_slots=1 << 16)
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="k must"):
            t1.indel_scan(s, 1, mixed=True)
    t1.close()
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    res = C.c_void_p()
    assert L.jasper_indel_scan_mixed(t._h, 1, cs, (C.c_int64 * 1)(-5), 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indel_scan_mixed(t._h, 1, cs, (C.c_int64 * 1)(200), 1, 4, None) != 0
    assert L.jasper_indel_scan_mixed(None, 1, cs, (C.c_int64 * 1)(200), 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indel_scan_mixed_device(t._h, 1, None, None, 1, 4, C.byref(res)) != 0 and not res
    assert L.jasper_indelscan_mixed_counts(None, 0, None) != 0 and L.jasper_indelscan_mixed_records(None, None, None) != 0
    # the mixed accessors of a plain result: zeros and n = 0
    assert L.jasper_indel_scan(t._h, 1, cs, (C.c_int64 * 1)(200), 1, 4, C.byref(res)) == 0 and res
    c3, rp, rn, nl = (C.c_uint64 * 3)(7, 7, 7), C.POINTER(_lib.MixedIns)(), C.c_uint64(9), C.c_uint64(9)
    assert L.jasper_indelscan_mixed_counts(res, 0, c3) == 0 and list(c3) == [0, 0, 0]
    assert L.jasper_indelscan_mixed_records(res, C.byref(rp), C.byref(rn)) == 0 and rn.value == 0
    assert L.jasper_indelscan_mixed_lookups(res, C.byref(nl)) == 0 and nl.value == 0
    assert L.jasper_indelscan_mixed_seconds(res) == 0.0 and L.jasper_indelscan_mixed_retried(res) == 0
    assert L.jasper_indelscan_mixed_counts(res, 1, c3) != 0
    L.jasper_indelscan_free(res)
    count = dict_counter(kmer_dict([b"ACGT" * 100], 31))
    check(t, seqs, 1, 16, restate_mixed(seqs, 31, count, 1, 16), "a period of four")
    t.close()
