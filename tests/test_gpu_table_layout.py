"""GPU: the table's layout rules at their limits, with keys placed by chosen hash (tests/layout_util.py).

Random reads at a load below 0.75 give probe sequences a handful of slots long.  Here the keys are crafted: KmerTable.import_entries
takes raw mixed hashes, the top bits of a hash are the key's home slot, and the library's inverse mix turns a chosen hash back
into a k-mer that can also be counted as bases and looked up as a string.  So a test can fill probe offsets 0 .. 1023 of one home,
wrap a chain around the table's end, push records across the end of a counting region, keep keys apart that differ in one half
of a wide remainder only, and hold counts of 2^32 and more.

Everything expected comes from a Python Counter keyed by canonical k-mer string (layout_util.Ref); every comparison is bit-exact:
the exported entries, info()["distinct"], the histogram, and lookup() of the keys and of absent keys that share a home, a tag
remainder or an ext word with present ones.  Nothing expected comes from the table under test.
"""
import os
import random
import re

import numpy as np
import pytest

import layout_util as lu
from layout_util import MAXPROBE, U32, Ref, absent_neighbours, check_table, craft, craft_edge, entries

pytestmark = pytest.mark.gpu

NARROW = [(17, 16), (31, 16), (32, 20), (37, 22)]        # (k, log2 slots): the whole remainder in the tag word
WIDE = [(37, 16), (45, 16), (64, 17)]                    # the low 64 remainder bits in the ext word (k = 37: all of them)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


def new_table(KT, k, s):
    t = KT(k, min_slots=1 << s)
    assert t.info()["slots"] == 1 << s
    assert (2 * k - s > 53) == lu.is_wide(k, s)
    return t


def check_parts(t, ref, nparts):
    """histogram_part: the parts sum to the histogram, and each is the reference filtered by the part-of-key function"""
    parts = [t.histogram_part(p, nparts) for p in range(nparts)]
    assert [sum(col) for col in zip(*parts)] == ref.histogram()
    for p in range(nparts):
        assert parts[p] == ref.filtered(lambda h: lu.part_of(ref.k, h, nparts) == p).histogram(), (p, nparts)


class env:
    """an environment variable for the duration of a block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- 1. the longest chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", NARROW + WIDE)
def test_longest_chain_then_growth(KT, k, s):
    """1024 keys of ONE home take probe offsets 0 .. 1023 (the tag's 10 offset bits, all values) and the table keeps its size;
    the 1025th key of that home has no slot, so the table grows, and nothing is lost.  Homes at the table's end: the chain wraps."""
    rng = random.Random(1000 * k + s)
    n = 1 << s
    for home in (n - 1, n - 512, 0, n // 3):
        hs, kms = craft(k, s, home, MAXPROBE + 1, rng)
        counts = [1 + (i * 7) % 13 for i in range(MAXPROBE)]
        ref = Ref(k).add_kmers(kms[:MAXPROBE], counts)
        absent = absent_neighbours(k, s, hs[:4] + hs[-4:], set(kms), rng)
        assert len(absent) >= 8
        t = new_table(KT, k, s)
        t.import_entries(entries(hs[:MAXPROBE], counts))
        assert t.info()["slots"] == n, "1024 keys of one home fit its probe sequence: no growth"
        check_table(t, ref, absent + kms[MAXPROBE:])
        t.import_entries(entries(hs[MAXPROBE:], [5]))
        ref.add_kmers(kms[MAXPROBE:], [5])
        assert t.info()["slots"] > n, "the 1025th key of one home must make the table grow"
        check_table(t, ref, absent)
        # the same chain through the counting kernel's insert
        t2 = new_table(KT, k, s)
        text = "N".join(kms[:MAXPROBE])
        t2.count_bases(text)
        assert t2.info()["slots"] == n
        check_table(t2, Ref(k).add_bases(text), absent, occurrences=MAXPROBE)
        t.close()
        t2.close()


# ---- 2. wide keys that differ in one half only ----------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", WIDE)
def test_wide_keys_that_differ_in_one_half(KT, k, s):
    """a wide slot's key is split into the tag's remainder bits and the ext word: keys of one home that share one of the two and
    differ in the other (by one bit, too) are different keys, and the combinations that were never inserted read 0"""
    rng = random.Random(2000 * k + s)
    rb = 2 * k - s
    tb, eb = max(0, rb - 64), min(64, rb)
    home = rng.randrange(1 << s)
    t0, e0 = rng.getrandbits(tb) if tb else 0, rng.getrandbits(eb)
    tags = list(dict.fromkeys([t0] + [t0 ^ (1 << b) for b in range(min(tb, 6))] + ([t0 ^ (1 << (tb - 1))] if tb else []) +
                              [rng.getrandbits(tb) for _ in range(30 if tb else 0)]))
    exts = list(dict.fromkeys([e0] + [e0 ^ (1 << b) for b in (0, 1, 2, 31, 32, 33, eb - 1)] + [rng.getrandbits(eb) for _ in range(32)]))
    grid = [(tg, ex) for tg in tags for ex in exts]
    hs, kms = craft(k, s, home, None, rng, rem=[(tg << 64) | ex for tg, ex in grid])
    is_present = lambda h: lu.split(k, s, h)[1] == t0 or lu.split(k, s, h)[2] == e0
    pres = [(h, km) for h, km in zip(hs, kms) if is_present(h)]
    absent = [km for h, km in zip(hs, kms) if not is_present(h)]
    assert len(pres) >= 16 and (len(absent) >= 100 or tb == 0)
    absent += absent_neighbours(k, s, [h for h, _ in pres[:8]], set(kms), rng)
    ph, pk = [h for h, _ in pres], [km for _, km in pres]
    t = new_table(KT, k, s)
    t.import_entries(entries(ph, [5] * len(ph)))
    ref = Ref(k).add_kmers(pk, [5] * len(pk))
    check_table(t, ref, absent)
    text = "N".join(pk)
    t.count_bases(text)
    ref.add_bases(text)
    assert all(c == 6 for c in ref.c.values())
    check_table(t, ref, absent, occurrences=len(pk))
    # the counting kernel inserts them, then finds them again
    t2 = new_table(KT, k, s)
    t2.count_bases(text)
    t2.count_bases(text + "N" + text)
    check_table(t2, Ref(k).add_bases(text, 3), absent, occurrences=3 * len(pk))
    assert t.info()["slots"] == t2.info()["slots"] == 1 << s
    t.close()
    t2.close()


# ---- 3. counts ------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 10000, 10001, 10002, 2**32 - 2, 2**32 - 1, 2**32, 2**40, 2**63]
TWICE = [(2**32 - 2, 1), (2**31, 2**31), (6000, 4001)]             # one key imported twice: the counts add


def check_derived(KT, t, ref, seqs):
    """what reads counts out of the table and clamps them: the parts' histograms, the dense report, the spectrum"""
    check_parts(t, ref, 3)
    for thre in (1, U32):
        rep = t.kmer_report(seqs, thre)
        want_counts, want_runs = ref.report(seqs, thre)
        assert rep.counts == want_counts and rep.run_tuples() == want_runs, thre
    keys = sorted(ref.c)
    asm_text = "N".join(keys[:8] + keys[:3] + [seqs[-1]])
    asm = KT(ref.k, min_slots=1 << 12)
    asm.count_bases(asm_text)
    assert t.spectrum(asm).cells.tolist() == ref.spectrum(Ref(ref.k).add_bases(asm_text))
    asm.close()


@pytest.mark.parametrize("k,s", [(31, 16), (37, 16)])
def test_counts_at_and_beyond_32_bits(KT, k, s, tmp_path):
    """counts of 2^32 and more stay exact in the table and are clamped to 2^32-1 wherever they are read out: lookup, both
    histograms (bin 10001 from 10001 on), the .jf file, the report (thresholds 1 and 2^32-1) and the spectrum"""
    rng = random.Random(3000 * k + s)
    hs, kms = craft(k, 0, 0, len(COUNTS) + len(TWICE) + 6, rng)
    n_in = len(COUNTS) + len(TWICE)
    absent = kms[n_in:] + absent_neighbours(k, s, hs[:n_in], set(kms), rng, per_key=1)
    t = new_table(KT, k, s)
    t.import_entries(entries(hs[:n_in], COUNTS + [a for a, _ in TWICE]))
    t.import_entries(entries(hs[len(COUNTS):n_in], [b for _, b in TWICE]))
    ref = Ref(k).add_kmers(kms[:n_in], COUNTS + [a + b for a, b in TWICE])
    assert sorted(ref.c.values())[-1] == 2**63 and ref.histogram()[10001] == 10 and ref.lookup([kms[6]]) == [U32]
    seqs = kms[:n_in] + ["N".join(kms[:n_in + 2]), kms[0].lower() + kms[5], kms[n_in]]
    check_table(t, ref, absent)
    check_derived(KT, t, ref, seqs)
    # the same keys counted as bases on top: 2^32-2 -> 2^32-1, 2^32-1 -> 2^32, 10000 -> 10001, ...
    text = "N".join(kms[:n_in])
    t.count_bases(text)
    ref.add_bases(text)
    assert ref.c[kms[4]] == U32 and ref.c[kms[5]] == 2**32 and ref.c[kms[8]] == 2**63 + 1
    check_table(t, ref, absent, occurrences=n_in)
    check_derived(KT, t, ref, seqs)
    # the .jf file stores min(count, 2^32-1)
    path = str(tmp_path / "big.jf")
    t.write_jf(path)
    back = KT.from_jf(path)
    assert back.k == k
    check_table(back, ref.clamped(), absent)
    back.close()
    import torch
    dev = torch.device("cuda", 0)
    from jasper_amd._lib import JasperHipError
    if k == 37:
        # 2k - 64 = 10 hash bits share the second word of a packed entry with the count: 54 count bits
        for top, fits in ((2**54 - 1, True), (2**54, False)):
            tp = new_table(KT, k, s)
            cs = [top, 1, 2**32, 10001]
            tp.import_entries(entries(hs[:4], cs))
            buf = torch.zeros((16, 2), dtype=torch.int64, device=dev)
            if not fits:
                with pytest.raises(JasperHipError, match="does not fit the packed exchange format"):
                    tp.export_packed(buf.data_ptr(), 16)
                tp.import_entries(entries(hs[4:6], [3, 4]))            # the refusal leaves the table as it was, and usable
                check_table(tp, Ref(k).add_kmers(kms[:6], cs + [3, 4]), absent)
                tp.close()
                continue
            assert tp.export_packed(buf.data_ptr(), 16) == 4
            assert sorted(lu.unpacked(k, buf, 4)) == sorted(zip(hs[:4], cs))
            tq = new_table(KT, k, s)
            tq.import_packed(buf.data_ptr(), 4)
            check_table(tq, Ref(k).add_kmers(kms[:4], cs), absent)
            tp.close()
            tq.close()
    else:
        # 2k <= 64: the whole second word is the count
        buf = torch.zeros((32, 2), dtype=torch.int64, device=dev)
        assert t.export_packed(buf.data_ptr(), 32) == n_in
        assert dict(lu.unpacked(k, buf, n_in)) == {h: ref.c[km] for h, km in zip(hs[:n_in], kms[:n_in])}
        tq = new_table(KT, k, s)
        tq.import_packed(buf.data_ptr(), n_in)
        check_table(tq, ref, absent)
        tq.close()
    t.close()


@pytest.mark.parametrize("k", [31, 37])
def test_polish_qv_counters_read_clamped_counts(KT, k):
    """the QV counters of a walk without fixing (bad = count < threshold, and the reference's comparisons of neighbouring counts)
    over sequences whose k-mers hold these counts, against the CPU oracle fed with the clamped counts"""
    from oracle import oracle
    rng = random.Random(3500 + k)
    seqs = ["".join(rng.choice("ACGT") for _ in range(6 * k + 17 * i)) for i in range(4)]
    cyc = COUNTS + [3, 2**33 + 1, 20000, 0, 2**32 + 7]
    ref, db, i = Ref(k), oracle.OracleDB(k), 0
    for sq in seqs:
        for j in range(len(sq) - k + 1):
            km = lu.canon(sq[j:j + k])
            if km not in ref.c and cyc[i % len(cyc)]:
                ref.add_kmers([km], [cyc[i % len(cyc)]])
            i += 1
    for km, c in ref.c.items():
        db.add_kmer(km, min(c, U32))
    t = new_table(KT, k, 16)
    keys = list(ref.c)
    t.import_entries(entries([lu.hash_of_kmer(km) for km in keys], [ref.c[km] for km in keys]))
    check_table(t, ref)
    names = ["s%d" % j for j in range(len(seqs))]
    for thre in (2, 10001, 2**31 - 1):
        got = t.polish_batch(seqs, thre, 2, fix=False)
        _, _, qv, _ = db.polish_batch(names, seqs, thre, 2, fix=False)
        assert got.qv == qv and got.seqs == seqs, thre
        assert qv[1] == sum(len(sq) - k + 1 for sq in seqs)
    t.close()


# ---- 4. growth and shrink ------------------------------------------------------------------------------------------------
CHAIN_HOMES = lambda n: (n - 1, n - 512, n // 2 + 77)


@pytest.mark.parametrize("k,s,s_big", [(31, 16, 18), (45, 16, 18), (37, 16, 22)])
def test_growth_and_shrink_keep_every_key(KT, k, s, s_big):
    """chains of 1024 keys (two of them overlapping and wrapping the table's end) plus spread keys: the import itself spills and
    grows; reserve rehashes into more slots; fit(0.5) rehashes into fewer, where the chains pile up, spill and make the table grow
    again.  k = 37: from a wide table (2^16) to one that keeps whole remainders in its tags (2^22).

    That every step succeeds follows from the layout, whatever order the GPU inserts in: no spread key is homed within a chain's
    1024 slots (at 2^16 slots, hence at any larger size), and from 2^18 slots on the overlapping chains' homes are 2044 slots
    apart, so every run of occupied slots that holds a chain is exactly 1024 long -- at most four rounds of growth, of the eight
    there are.  (A chain on home 0 next to the one on home n-1 would be 2048 keys on adjacent homes, which stay adjacent however
    often the table doubles: the cluster that cannot be split has the test below.)"""
    rng = random.Random(4000 * k + s)
    n = 1 << s
    hs, kms = [], []
    for home in CHAIN_HOMES(n):
        a, b = craft(k, s, home, MAXPROBE, rng)
        hs += a
        kms += b
    n_chain = len(hs)
    near = lambda h: any(((h >> (2 * k - s)) - home + 16) % n < MAXPROBE + 32 for home in CHAIN_HOMES(n))
    a, b = craft(k, 0, 0, 3400, rng)
    keep = [i for i, h in enumerate(a) if not near(h)][:3000]
    assert len(keep) == 3000
    hs += [a[i] for i in keep]
    kms += [b[i] for i in keep]
    assert len(set(kms)) == len(kms)
    counts = [1 + (i * 11) % 10005 for i in range(len(hs))]
    ref = Ref(k).add_kmers(kms, counts)
    absent = absent_neighbours(k, s, hs[:3] + hs[2047:2050] + hs[-3:], set(kms), rng)
    t = new_table(KT, k, s)
    t.import_entries(entries(hs, counts))
    assert t.info()["slots"] >= 1 << 18, "chains that overlap at 2^16 and 2^17 slots: the import had to grow the table"
    check_table(t, ref, absent)
    t.reserve(1 << (s_big + 2))
    assert t.info()["slots"] == 1 << (s_big + 2) and lu.is_wide(k, s_big + 2) == (k == 45)
    check_table(t, ref, absent)
    t.fit(0.5)
    assert 1 << 18 <= t.info()["slots"] < 1 << (s_big + 2), "fit went below what the chains need, spilled and grew again"
    check_table(t, ref, absent)
    t.import_entries(entries(hs[:100] + hs[n_chain:n_chain + 100], [2**32] * 200))        # ... and the table goes on working
    ref.add_kmers(kms[:100] + kms[n_chain:n_chain + 100], [2**32] * 200)
    check_table(t, ref, absent)
    t.close()


def test_cluster_that_growth_cannot_split(KT):
    """about 1100 keys that share their top 40 hash bits share a home in every table of up to 2^40 slots: eight rounds of growth
    cannot give them 1100 slots.  The import raises an error or holds every key -- it never succeeds with keys missing -- and a
    table created afterwards works."""
    from jasper_amd._lib import JasperHipError
    k, s = 31, 16
    rng = random.Random(4100)
    hs, kms = craft(k, 40, rng.getrandbits(40), 1100, rng)
    ref = Ref(k).add_kmers(kms, [3] * len(kms))
    t = new_table(KT, k, s)
    try:
        t.import_entries(entries(hs, [3] * len(hs)))
    except JasperHipError as e:
        assert "table" in str(e)
    else:
        check_table(t, ref)
    t.close()
    t2 = new_table(KT, k, s)
    a, b = craft(k, 0, 0, 500, rng)
    t2.import_entries(entries(a, [2] * 500))
    check_table(t2, Ref(k).add_kmers(b, [2] * 500))
    t2.close()


# ---- 5. partitions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [2, 3, 7, 8])
def test_partitions_whose_chains_end_in_the_next_range(KT, nparts):
    """a key belongs to partition floor(top32(hash) nparts / 2^32) wherever its slot is: a full chain (1024 keys, probe offsets up to
    1023) on the LAST home slot of a partition's range lies in the next partition's range (the last one wraps to slot 0), and the
    scan of a partition's slots has to go 1023 slots past its last home to find all of it.  With 3 and 7 partitions that home's
    keys belong to two partitions.  (No spread key is homed within a chain's slots, so that the chains are exactly full.)"""
    import torch
    k, s = 37, 20
    n = 1 << s
    rng = random.Random(5000 + nparts)
    hs, kms = [], []
    homes = [lu.last_home_of_part(s, p, nparts) for p in range(nparts)]
    for home in homes:
        a, b = craft(k, s, home, MAXPROBE, rng)
        hs += a
        kms += b
    near = lambda h: any(((h >> (2 * k - s)) - home + 16) % n < MAXPROBE + 32 for home in homes)
    a, b = craft(k, 0, 0, 3400, rng)
    keep = [i for i, h in enumerate(a) if not near(h)][:3000]
    assert len(keep) == 3000
    hs += [a[i] for i in keep]
    kms += [b[i] for i in keep]
    assert len(set(kms)) == len(kms)
    counts = [1 + (i * 13) % 10007 for i in range(len(hs))]
    ref = Ref(k).add_kmers(kms, counts)
    t = new_table(KT, k, s)
    t.import_entries(entries(hs, counts))
    assert t.info()["slots"] == 1 << s
    check_table(t, ref, absent_neighbours(k, s, hs[:2] + hs[1023:1025] + hs[-2:], set(kms), rng))
    check_parts(t, ref, nparts)
    dev = torch.device("cuda", 0)
    sizes = []
    for p in range(nparts):
        want = {h: c for h, c in zip(hs, counts) if lu.part_of(k, h, nparts) == p}
        assert len(want) >= 900
        n = t.export_packed(0, 0, p, nparts)
        buf = torch.zeros((n + 8, 2), dtype=torch.int64, device=dev)
        assert t.export_packed(buf.data_ptr(), n + 8, p, nparts) == n
        got = lu.unpacked(k, buf, n)
        assert len(got) == len(dict(got)) and dict(got) == want, p
        assert not buf[n:].any(), "nothing is written past the entries"
        sizes.append(n)
    assert sum(sizes) == ref.distinct == t.info()["distinct"]
    t.close()


# ---- 6. region-wise import ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(31, 16), (37, 22)])
def test_region_wise_import_of_packed_lists(KT, k, s, capfd):
    """import_packed_multi into an empty table builds it region by region (4096 slots each) in LDS; an entry whose probe sequence
    leaves its region, or that is not where the list order says, takes the deferred list.  Lists with more keys homed in a region's
    last 16 slots than fit there (the table's last region among them), out-of-order stretches, a key in two lists, zero counts."""
    import torch
    dev = torch.device("cuda", 0)
    rng = random.Random(6000 * k + s)
    R, nreg = 4096, 1 << (s - 12)
    groups = [craft_edge(k, s, (reg + 1) * R - 16, 16, 80, rng) for reg in (3, nreg // 2, nreg - 1)]
    spread = craft(k, 0, 0, 6000, rng)
    zeros = craft(k, 0, 0, 50, rng)
    hs = [h for g in groups for h in g[0]] + spread[0]
    kms = [km for g in groups for km in g[1]] + spread[1]
    assert len(set(kms)) == len(kms) and not set(zeros[1]) & set(kms)
    key_of = dict(zip(hs, kms))
    lists = [[], [], []]
    for i, h in enumerate(hs):
        c = 1 + (i * 17) % 10003
        lists[i % 3].append((h, c))
        if i % 5 == 0:
            lists[(i + 1) % 3].append((h, 2**32 + i))          # the same key in two lists
        if i % 40 == 0:
            lists[(i + 2) % 3].append((h, 0))                  # ... and as a zero-count entry in a third
    for j, h in enumerate(zeros[0]):
        lists[j % 3].append((h, 0))                            # keys that only ever come with count 0 do not exist
    ref = Ref(k)
    for L in lists:
        L.sort()                                               # slot order = hash order
        ref.add_kmers([key_of[h] for h, c in L if c], [c for h, c in L if c])
    lists[0][100:400] = lists[0][100:400][::-1]                # out-of-order stretches
    lists[1][:200], lists[1][-200:] = lists[1][-200:], lists[1][:200]
    tens = [lu.packed_tensor(k, L, dev) for L in lists]
    absent = zeros[1] + absent_neighbours(k, s, hs[:6] + hs[237:240], set(kms) | set(zeros[1]), rng)
    tables = []
    for atomic in (False, True):
        t = new_table(KT, k, s)
        with env(JASPER_COUNT_DEBUG="1", **({"JASPER_IMPORT_ATOMIC": "1"} if atomic else {})):
            t.import_packed_multi([x.data_ptr() for x in tens], [len(L) for L in lists])
        log = capfd.readouterr().err
        m = re.search(r"\[import\] (\d+) entries into (\d+) LDS regions, (\d+) deferred", log)
        assert (m is None) == atomic, log[-300:]
        if m:
            print("region-wise import k=%d: %s" % (k, m.group(0)))
            # 80 keys homed in a region's last 16 slots: at least 64 of them leave it, in each of the three regions
            assert int(m.group(2)) == nreg and int(m.group(3)) >= 3 * 64
        assert t.info()["slots"] == 1 << s
        check_table(t, ref, absent)
        tables.append(t)
    assert lu.table_dict(tables[0]) == lu.table_dict(tables[1])
    for t in tables:
        t.close()


# ---- 7. partitioned counting at region edges -------------------------------------------------------------------------------------
REPEATS = 30
FILLER_BASES, FILLER_TILES = 200_000, 42


def _stream(k, s, rbits):
    """(bases as a numpy uint8 array, reference of one pass over them, crafted groups): filler reads of a small genome, and crafted
    canonical k-mers as `kmer + "N"` units, REPEATS times each, between the filler's tiles"""
    rng = random.Random(7000 + k)
    groups = lu.region_edge_keys(k, s, rbits, rng)
    genome = "".join(rng.choice("ACGT") for _ in range(FILLER_BASES))
    filler = "".join(genome[i:i + 150] + "N" for i in range(0, FILLER_BASES, 150))
    crafted = "".join(km + "N" for g in groups.values() for km in g[1])
    fa, ca = np.frombuffer(filler.encode(), dtype=np.uint8), np.frombuffer(crafted.encode(), dtype=np.uint8)
    pieces = []
    for i in range(FILLER_TILES):
        pieces.append(fa)
        if i < REPEATS:
            pieces.append(ca)
    ref = Ref(k).add_bases(filler, FILLER_TILES).add_bases(crafted, REPEATS)
    return np.concatenate(pieces), ref, groups


@pytest.mark.parametrize("k", [37, 38, 41, 51])
def test_partitioned_counting_at_region_edges(KT, k, capfd):
    """the atomic-free counting path builds the table region by region in LDS; a record whose probe sequence leaves its region is
    deferred to the direct path.  Crafted keys make that happen by pigeonhole: 64 keys homed in the last 16 slots of a region (of
    the table's last region; of a region whose successor's first slots are taken), a 600-key chain across a region's end.  k = 37:
    8-byte records; k = 38: 16-byte records into a table with whole remainders in its tags; k = 41, 51: 16-byte records into a
    wide table.  Expected counts come from the string Counter of the stream alone."""
    import torch
    s = 24
    wide = lu.is_wide(k, s)
    rbits = 11 if wide else 12
    bases, ref, groups = _stream(k, s, rbits)
    assert bases.size >= 8 << 20 and bases.size < 0.7 * (1 << s)
    d = torch.from_numpy(bases).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    crafted_h = [h for g in groups.values() for h in g[0]]
    crafted_k = [km for g in groups.values() for km in g[1]]
    assert all(ref.c[km] == REPEATS for km in crafted_k)
    absent = absent_neighbours(k, s, [g[0][0] for g in groups.values()] + [g[0][-1] for g in groups.values()], set(crafted_k), rng=random.Random(k))
    absent = [km for km in absent if km not in ref.c]
    sample = crafted_k + list(ref.c)[::16]

    def count(t, partitioned=True):
        with env(JASPER_COUNT_DEBUG="2"):
            t.count_bases_device(d.data_ptr(), d.numel())
        log = capfd.readouterr().err
        assert "piece abandoned" not in log, log[-400:]
        assert t.info()["slots"] == 1 << s
        if not partitioned:
            assert t.count_path() == 0 and t.count_stages()[1] == 0
            return None
        assert t.count_path() == 1 and t.count_stages()[1] >= 1, "the partitioned path was not taken"
        m = re.search(r"rbits (\d+) .* deferred (\d+)", log)
        assert m and int(m.group(1)) == rbits, log[-400:]
        # three clusters of 64 keys on 16 slots: at least 48 keys each leave their region, REPEATS records per key
        assert int(m.group(2)) >= 3 * 48 * REPEATS
        return int(m.group(2))

    # into an empty table: the fused histogram, then the table's own
    t = new_table(KT, k, s)
    deferred = [count(t)]
    assert t.histogram_is_fused() == (not wide)
    assert t.histogram() == ref.histogram()
    check_table(t, ref, absent, present=sample, occurrences=ref.occurrences)
    t.import_entries(entries(crafted_h[:1], [0]))              # (changes nothing, drops the fused histogram)
    assert not t.histogram_is_fused() and t.histogram() == ref.histogram()
    # a second call on the same table
    deferred.append(count(t))
    ref2 = ref.copy().add_counter(ref.c)
    check_table(t, ref2, absent, present=sample, occurrences=2 * ref.occurrences)
    t.close()
    # into a table that already holds the crafted keys
    t = new_table(KT, k, s)
    t.import_entries(entries(crafted_h, [7] * len(crafted_h)))
    deferred.append(count(t))
    check_table(t, ref.copy().add_kmers(crafted_k, [7] * len(crafted_k)), absent, present=sample, occurrences=ref.occurrences)
    t.close()
    # the direct kernel
    t = new_table(KT, k, s)
    with env(JASPER_COUNT_DIRECT="1"):
        count(t, partitioned=False)
    check_table(t, ref, absent, present=sample, occurrences=ref.occurrences)
    t.close()
    print("partitioned counting k=%d: %d bases, %d distinct, regions of 2^%d, deferred records (empty table, second call, pre-filled): %s"
          % (k, bases.size, ref.distinct, rbits, deferred))
