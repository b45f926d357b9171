"""GPU: the variant scan (KmerTable.variant_scan / variant_scan_device, jasper_variant_scan) against a restatement of its semantics
fed by Python dicts of canonical k-mer strings: the dict of a golden case's dump.txt.gz (printed by the real `jellyfish dump -c`) or a
dict of the reads' canonical k-mers.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): position p of a sequence s of n bytes is evaluated iff k-1 <= p <= n-k and all 2k-1 bytes
s[p-k+1 .. p+k-1] are ACGTacgt; m(p, x) = the minimum over the k windows that cover p of the count of the window's canonical k-mer with
byte p replaced by x, clamped to 2^32-1; ref = the folded s[p]; for every x != ref with m(p, x) >= thre one record (seq, p, ref, x,
m(p, ref), m(p, x), kind), kind 1 (het) when m(p, ref) >= thre, else 2 (error); ordered by (seq, pos, alt); per sequence (evaluated,
het, error).  A candidate -- what the dense scan hands to the check -- is a valid window (all k bytes bases) that ends at p, with any
p >= k-1, whose k-mer with the last base replaced by x != s[p] has a count >= thre."""
import numpy as np
import pytest

from golden_util import Case, case_names
from test_gpu_copies import TILE, as_bytes, dict_counter, is_wide, kmer_dict

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
HET, ERROR = 1, 2
ACGT = b"ACGT"


def restate(seqs, k, count, thre):
    """(counts, records, candidates) of the semantics above; count(bytes of k upper-case bases) -> int.  `all terms >= thre` stands
    for `minimum >= thre`, so an alternative is left at its first window below thre"""
    counts, recs, ncand = [], [], 0
    for si, s in enumerate(seqs):
        b = as_bytes(s)
        n = len(b)
        up = b.upper()
        pre = [0] * (n + 1)
        for i, ch in enumerate(b):
            pre[i + 1] = pre[i] + (0 if ch in b"ACGTacgt" else 1)
        ev = het = err = 0
        for p in range(k - 1, n):
            w = p - k + 1
            if pre[p + 1] != pre[w]:
                continue                                  # the window that ends at p is not valid
            ref = up[p:p + 1]
            alts = [bytes([x]) for x in ACGT if bytes([x]) != ref]
            solid0 = [x for x in alts if min(count(up[w:p] + x), U32) >= thre]
            ncand += len(solid0)
            if p > n - k or pre[p + k] != pre[w]:
                continue                                  # not evaluated
            ev += 1
            for x in solid0:
                amin = U32
                for j in range(k):
                    c = min(count(up[w + j:p] + x + up[p + 1:w + j + k]), U32)
                    amin = min(amin, c)
                    if c < thre:
                        break
                if amin < thre:
                    continue
                rmin = min(min(count(up[w + j:w + j + k]), U32) for j in range(k))
                kind = HET if rmin >= thre else ERROR
                recs.append((si, p, ref.decode(), x.decode(), rmin, amin, kind))
                het += kind == HET
                err += kind == ERROR
        counts.append((ev, het, err))
    return counts, recs, ncand


def restate_plain(seqs, k, count, thre):
    """the same without any shortcut (every minimum over all k windows, every alternative): for small inputs, to check `restate`"""
    counts, recs = [], []
    for si, s in enumerate(seqs):
        b = as_bytes(s)
        n, up = len(b), as_bytes(s).upper()
        ev = het = err = 0
        for p in range(k - 1, n - k + 1):
            if any(ch not in b"ACGT" for ch in up[p - k + 1:p + k]):
                continue
            ev += 1
            m = {x: min(min(count(up[w:p] + bytes([x]) + up[p + 1:w + k]), U32) for w in range(p - k + 1, p + 1)) for x in ACGT}
            for x in ACGT:
                if x != up[p] and m[x] >= thre:
                    kind = HET if m[up[p]] >= thre else ERROR
                    recs.append((si, p, chr(up[p]), chr(x), m[up[p]], m[x], kind))
                    het += kind == HET
                    err += kind == ERROR
        counts.append((ev, het, err))
    return counts, recs


def summary(counts, recs):
    return sum(c[1] for c in counts), sum(c[2] for c in counts)


def check(vs, want, what):
    want_counts, want_recs, want_cand = want
    assert vs.counts == want_counts, what
    got = vs.record_tuples()
    assert len(got) == len(want_recs), (what, len(got), len(want_recs))
    assert got == want_recs, what
    assert vs.candidates == want_cand, (what, vs.candidates, want_cand)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


def rand_bases(rng, n):
    return np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def other_base(ch, step=1):
    return ACGT[(ACGT.index(bytes([ch]).upper()) + step) % 4:][:1]


def substituted(s, sites, step=1):
    t = bytearray(s)
    for p in sites:
        t[p:p + 1] = other_base(s[p], step)
    return bytes(t)


# ---- golden cases ------------------------------------------------------------------------------------------------------------------
# (het, error, candidates) from the restatement over the committed dumps, computed on the CPU
ANCHORS = {"diploid_k25": (10, 0, 13), "rolling_k25": (2, 2, 20), "rolling_k37": (2, 2, 20), "cluster_k25": (0, 4, 13), "gaps_k37_p4": (0, 6, 32),
           "simple_k63": (0, 4, 9)}
_golden_seen = {}


def golden_expected(c):
    _, seqs = c.batch()
    rd = {key.encode(): v for key, v in c.dump().items()}
    return seqs, restate(seqs, c.k, dict_counter(rd), c.thre)


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    seqs, want = golden_expected(c)
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    vs = t.variant_scan(seqs, c.thre)
    t.close()
    het, err = summary(want[0], want[1])
    print(name, (het, err, want[2]), summary(vs.counts, vs.record_tuples()) + (vs.candidates,))
    check(vs, want, name)
    if name in ANCHORS:
        assert (het, err, want[2]) == ANCHORS[name]
    assert vs.seconds > 0 and not vs.retried
    _golden_seen[name] = (het, err, want[2])


def test_golden_cases_hold_every_kind():
    """(runs after the cases above) het records, error records, and candidates the check rejects all occur"""
    assert set(ANCHORS) <= set(case_names())
    seen = _golden_seen or {n: ANCHORS[n] for n in ANCHORS}
    assert any(h > 0 for h, _, _ in seen.values()) and any(e > 0 for _, e, _ in seen.values())
    assert any(c > h + e for h, e, c in seen.values())
    assert all(c > h + e for h, e, c in ANCHORS.values())


# ---- constructed edges -------------------------------------------------------------------------------------------------------------
def edges_workload():
    k, thre = 31, 5
    rng = np.random.default_rng(4631)
    n = 4 * TILE
    h1 = rand_bases(rng, n)
    sites = [k - 1, 4095, 4096 + k - 1, 8191 + k - 1, 12288, n - k]
    h2 = substituted(h1, sites)
    fake = h1[10000 - k + 1:10000] + other_base(h1[10000], 2)            # the single k-mer that ends at 10000 with another base
    reads = [h1] * 10 + [h2] * 8 + [fake] * 6
    asm = substituted(h1, [2000, 6000], 3)
    asm = asm[:5000].lower() + asm[5000:]
    seqs = [asm]
    # a 300-base pair of haplotypes whose differences are one position outside the evaluated range on either side
    a1 = rand_bases(rng, 300)
    a2 = substituted(a1, [k - 2, 300 - k + 1])
    reads += [a1] * 10 + [a2] * 8
    seqs.append(a1)
    # a site at 150 with N at 150 + k - 1 (not evaluated), and with n at 150 + k (evaluated: one het record)
    b1 = rand_bases(rng, 400)
    b2 = substituted(b1, [150])
    reads += [b1] * 10 + [b2] * 8
    seqs.append(b1[:150 + k - 1] + b"N" + b1[150 + k:])
    seqs.append(b1[:150 + k] + b"n" + b1[150 + k + 1:])
    seqs.append(rand_bases(rng, 40))
    seqs.append(b"")
    return k, thre, sites, reads, seqs


def test_constructed_edges(KT):
    k, thre, sites, reads, seqs = edges_workload()
    rd = kmer_dict(reads, k)
    count = dict_counter(rd)
    want = restate(seqs, k, count, thre)
    counts, recs, ncand = want
    first = [r for r in recs if r[0] == 0]
    n = len(seqs[0])
    assert [r[1] for r in first] == sorted(sites + [2000, 6000]) and len(first) == 8
    assert all(r[4:] == (10, 8, HET) for r in first if r[1] in sites) and all(r[4:] == (0, 18, ERROR) for r in first if r[1] in (2000, 6000))
    assert counts[0] == (n - 2 * k + 2, 6, 2)
    assert restate([seqs[0]], k, count, thre)[2] == 9                  # the eight sites and the k-mer that ends at 10000
    assert counts[1] == (300 - 2 * k + 2, 0, 0) and restate([seqs[1]], k, count, thre)[2] == 1       # p = n - k + 1: a candidate, not evaluated
    assert counts[2] == (400 - 2 * k + 2 - (2 * k - 1), 0, 0) and counts[3] == (400 - 2 * k + 2 - (2 * k - 1), 1, 0)
    assert [r[:2] for r in recs if r[0] == 3] == [(3, 150)]
    assert counts[4] == (0, 0, 0) and counts[5] == (0, 0, 0)
    assert len(recs) == 9 and ncand > len(recs)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    vs = t.variant_scan(seqs, thre)
    print(vs.counts, vs.candidates, ncand)
    check(vs, want, "edges")
    t.close()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
FUZZ_KS = [1, 2, 5, 16, 17, 31, 32, 33, 37, 63, 64]


def fuzz_workload(k):
    """a few sequences of at most 10 000 bytes with N runs and lower case; reads = copies of them with substitutions of their own, so
    that every threshold 1..4 separates some alleles from others"""
    rng = np.random.default_rng(9100 + k)
    g = rand_bases(rng, 10_000)
    reads = []
    for copies, nsub in ((3, 40), (2, 40), (1, 40), (1, 40)):
        h = substituted(g, sorted(rng.choice(len(g), nsub, replace=False).tolist()), int(rng.integers(1, 4)))
        reads += [h] * copies
    a = bytearray(substituted(g, sorted(rng.choice(len(g), 30, replace=False).tolist()), 2))
    for p in rng.integers(0, len(a) - 40, 4).tolist():
        a[p:p + int(rng.integers(1, 30))] = b"N" * 1
    lo = int(rng.integers(0, len(a) - 2000))
    a[lo:lo + 1500] = bytes(a[lo:lo + 1500]).lower()
    for p, ch in zip(rng.integers(0, len(a), 6).tolist(), b"nRY-*x"):
        a[p] = ch
    a = bytes(a)
    seqs = [a, g[3000:3000 + TILE + 2 * k], b"", g[100:100 + 2 * k - 2], g[200:200 + 2 * k - 1], g[300:300 + 2 * k].lower(), g[5000:5000 + TILE + k - 1]]
    for _ in range(20):
        p = int(rng.integers(0, len(a) - 300))
        seqs.append(a[p:p + int(rng.integers(0, 300))])
    return reads, seqs


@pytest.mark.parametrize("k", FUZZ_KS)
def test_fuzz_against_dicts(KT, k):
    import torch
    reads, seqs = fuzz_workload(k)
    assert max(len(s) for s in seqs) <= 10_000
    rd = kmer_dict(reads, k)
    count = dict_counter(rd)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    if k >= 37:
        assert is_wide(t)
    if k <= 32:
        assert not is_wide(t)
    kinds = set()
    for thre in (1, 2, 3, 4):
        want = restate(seqs, k, count, thre)
        vs = t.variant_scan(seqs, thre)
        print(k, thre, summary(want[0], want[1]), want[2], summary(vs.counts, vs.record_tuples()), vs.candidates)
        check(vs, want, (k, thre))
        kinds |= {r[6] for r in want[1]}
        assert sum(c[0] for c in want[0]) > 5000
    assert kinds == ({HET, ERROR} if k >= 16 else {HET})      # (small k: every k-mer is in the reads, so every base is solid)
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.variant_scan_device(d, offs, 2) == t.variant_scan(seqs, 2)      # host text and device text give the same object
    t.close()


def test_the_restatement_agrees_with_its_plain_form():
    """(no GPU needed, it only guards the shortcut in `restate`)"""
    for k in (1, 2, 5):
        reads, seqs = fuzz_workload(k)
        seqs = [s[:600] for s in seqs[:8]]
        count = dict_counter(kmer_dict(reads, k))
        for thre in (1, 3):
            counts, recs, _ = restate(seqs, k, count, thre)
            assert (counts, recs) == restate_plain(seqs, k, count, thre)


# ---- other cases -------------------------------------------------------------------------------------------------------------------
def small_workload(seed, k, G=20_000):
    rng = np.random.default_rng(seed)
    h1 = rand_bases(rng, G)
    h2 = substituted(h1, list(range(97, G - 97, 211)))
    reads = [h1] * 6 + [h2] * 5
    asm = substituted(h1, list(range(1000, G - 1000, 1777)), 2)
    seqs = [asm, asm[2000:9000].lower(), b"", asm[:2 * k - 2], h2[3000:3000 + TILE + 3 * k], asm[500:900] + b"N" + asm[901:1400]]
    return reads, seqs


@pytest.mark.parametrize("slots,wide", [(1 << 16, True), (1 << 22, False)])
def test_narrow_against_wide(KT, slots, wide):
    """k = 37 is wide below 2^21 slots and narrow from there on: the same workload in tables of two sizes, the same result"""
    k = 37
    reads, seqs = small_workload(77, k)
    want = restate(seqs, k, dict_counter(kmer_dict(reads, k)), 3)
    assert {r[6] for r in want[1]} == {HET, ERROR} and len(want[1]) > 50
    t = KT(k, min_slots=slots)
    t.count_bases(b"N".join(reads))
    assert is_wide(t) == wide
    check(t.variant_scan(seqs, 3), want, slots)
    t.close()


@pytest.mark.parametrize("nshard", [2, 3])
def test_scan_through_owner_shards_equals_whole_table(KT, nshard):
    from test_gpu_shard import make_shards
    k = 37
    reads, seqs = small_workload(321, k, G=60_000)
    full = KT(k, min_slots=1 << 21)
    full.count_bases(b"N".join(reads))
    shards, _ = make_shards(KT, full, nshard, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    want = full.variant_scan(seqs, 3)
    assert {r[6] for r in want.record_tuples()} == {HET, ERROR} and len(want.records) > 100 and want.candidates >= len(want.records)
    for t in shards:
        assert t.variant_scan(seqs, 3) == want
    for t in shards + [full]:
        t.close()


def test_more_candidates_than_the_first_buffer_holds(KT):
    """k = 4, a random 40 000-base sequence counted as its own reads, thre 1: all 136 canonical 4-mers are present, so every
    alternative of every position is solid -- three records per evaluated position, more than the first list (windows / 64 + 65 536)"""
    k = 4
    s = rand_bases(np.random.default_rng(404), 40_000)
    rd = kmer_dict([s], k)
    assert len(rd) == 136 and min(rd.values()) >= 100
    want = restate([s], k, dict_counter(rd), 1)
    assert want[0] == [(39_994, 119_982, 0)] and want[2] == 3 * (40_000 - k + 1) and len(want[1]) == 119_982 > (40_000 - k + 1) // 64 + 65_536 == 66_160
    t = KT(k, min_slots=1 << 16)
    t.count_bases(s)
    vs = t.variant_scan([s], 1)
    check(vs, want, "dense")
    assert vs.retried
    vs = t.variant_scan([s], max(rd.values()) + 1)
    assert vs.counts == [(39_994, 0, 0)] and vs.candidates == 0 and not vs.retried and len(vs.records) == 0
    t.close()


def test_ten_calls_and_interleaved_scans_keep_their_results_and_leave_the_table_alone(KT):
    from test_gpu_copies import asm_table, histo_of, peak_rule
    k = 31
    reads, seqs = small_workload(9, k, G=50_000)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join(reads))
    a = asm_table(KT, k, seqs)
    before = t.info(), list(t.histogram())
    first = t.variant_scan(seqs, 3)
    assert len(first.records) > 100
    peak = peak_rule(histo_of(kmer_dict(reads, k)), 3)
    krep, crep = t.kmer_report(seqs, 3), t.copy_report(a, seqs, 3, peak)
    for _ in range(9):
        assert t.variant_scan(seqs, 3) == first
    # a report, a copy scan and a variant scan of one table keep their own buffers
    assert t.kmer_report(seqs, 3) == krep
    assert t.variant_scan(seqs, 3) == first
    assert t.copy_report(a, seqs, 3, peak) == crep
    assert t.variant_scan(seqs[:2], 3).counts == first.counts[:2]
    assert t.kmer_report(seqs, 3) == krep and t.copy_report(a, seqs, 3, peak) == crep
    assert (t.info(), list(t.histogram())) == before
    t.close()
    a.close()


def test_bad_arguments_are_errors(KT):
    import ctypes as C
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    with pytest.raises(_lib.JasperHipError, match="threshold"):
        t.variant_scan(seqs, 0)
    with pytest.raises(_lib.JasperHipError, match="threshold"):
        t.variant_scan([], 0)                                 # (also with nothing to scan)
    L = _lib.lib()
    cs = (C.c_char_p * 1)(b"ACGT" * 50)
    res = C.c_void_p()
    assert L.jasper_variant_scan(t._h, 1, cs, (C.c_int64 * 1)(-5), 1, C.byref(res)) != 0 and not res           # a negative length
    assert L.jasper_variant_scan(t._h, 1, cs, (C.c_int64 * 1)(200), 1, None) != 0                              # a null output
    assert L.jasper_variant_scan(None, 1, cs, (C.c_int64 * 1)(200), 1, C.byref(res)) != 0 and not res
    assert L.jasper_variant_scan_device(t._h, 1, None, (C.c_int64 * 2)(10, 5), 1, C.byref(res)) != 0 and not res   # offsets that decrease
    assert L.jasper_variant_scan_device(t._h, 1, None, None, 1, C.byref(res)) != 0 and not res
    assert t.variant_scan(seqs, 1).counts == [(200 - 2 * 31 + 2, 0, 0)]
    t.close()


def test_an_empty_table_gives_no_record(KT):
    k = 31
    reads, seqs = small_workload(10, k)
    want_ev = restate(seqs, k, lambda km: 0, 1)[0]
    empty = KT(k, min_slots=1 << 16)                  # never counted into: logically empty, its memory was never written
    vs = empty.variant_scan(seqs, 1)
    assert vs.counts == want_ev and sum(c[0] for c in want_ev) > 20_000 and len(vs.records) == 0 and vs.candidates == 0
    empty.count_bases(b"N".join(reads))
    empty.clear()                                     # cleared: logically empty again
    vs = empty.variant_scan(seqs, 1)
    assert vs.counts == want_ev and len(vs.records) == 0 and vs.candidates == 0
    assert empty.variant_scan([], 1).counts == [] and empty.variant_scan(["", "ACG"], 1).counts == [(0, 0, 0)] * 2
    empty.close()
