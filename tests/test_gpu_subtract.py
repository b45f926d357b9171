"""GPU: KmerTable.subtract (jasper_table_subtract, csrc/select.hip) against a restatement on Python dicts of canonical k-mer strings.
The tables are filled with keys placed by chosen hash (tests/layout_util.py: craft, craft_edge, entries), so a test decides which slots,
chains and piece edges the sweep meets; nothing expected here comes from the code under test.

Compared, bit-exact: the destination's exported entries (key -> 64-bit difference), the five counters and `missing`, both sources
unchanged, info()["distinct"], and lookup() of the dropped keys (0)."""
import os
import random

import pytest

import layout_util as lu
from layout_util import MAXPROBE, U32, craft, craft_edge, entries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


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


def filled(KT, k, s, d):
    """a table of 2^s slots holding the dict d (canonical k-mer string -> count); it must not have grown"""
    t = KT(k, min_slots=1 << s)
    assert t.info()["slots"] == 1 << s
    if d:
        t.import_entries(entries([lu.hash_of_kmer(km) for km in d], list(d.values())))
    info = t.info()
    assert info["slots"] == 1 << s and info["distinct"] == len(d)
    return t


def restate(sd, md):
    """src - minus on dicts -> (the difference, (swept, matched, dropped, underflow, kept), missing)"""
    want = {km: c - md.get(km, 0) for km, c in sd.items() if c > md.get(km, 0)}
    matched = sum(1 for km in sd if km in md)
    dropped = sum(1 for km, c in sd.items() if md.get(km, 0) == c)
    underflow = sum(1 for km, c in sd.items() if md.get(km, 0) > c)
    return want, (len(sd), matched, dropped, underflow, len(want)), len(md) - matched


def check_subtract(KT, src, minus, sd, md):
    want, counters, missing = restate(sd, md)
    dst, st = KT.subtract(src, minus)
    try:
        got = lu.table_dict(dst)
        assert got == want, lu._diff(got, want)
        assert (st["swept"], st["matched"], st["dropped"], st["underflow"], st["kept"]) == counters
        assert st["missing"] == missing
        assert dst.info()["distinct"] == len(want) and dst.k == src.k
        assert dst.info()["occurrences"] == sum(want.values()) % 2**64      # (the sum of the differences)
        assert st["seconds"] > 0
        gone = [km for km in sd if km not in want][:2000] + [km for km in md if km not in want][:500]
        assert dst.lookup(gone) == [0] * len(gone)
        keys = list(want)[:2000]
        assert dst.lookup(keys) == [min(want[km], U32) for km in keys]
    finally:
        dst.close()
    # the sources are what they were
    assert lu.table_dict(src) == sd and lu.table_dict(minus) == md
    return want, counters, missing


def close(*tables):
    for t in tables:
        t.close()


def mixed_minus(kms, sd, rng_extra=()):
    """a minus that meets every class: a third of the keys with less than src's count where there is less, a sixth with the same, a
    few with more, and keys src lacks"""
    md = {}
    for i, km in enumerate(kms):
        if i % 3 == 0 and sd[km] > 1:
            md[km] = sd[km] - 1 - (i % 2 if sd[km] > 2 else 0)
        elif i % 6 == 1:
            md[km] = sd[km]
        elif i % 41 == 2:
            md[km] = sd[km] + 1 + i % 3
    md.update({km: 2 for km in rng_extra})
    return md


@pytest.mark.parametrize("k", [21, 41])
def test_chain_that_wraps_in_source_and_minus(KT, k):
    """1000 keys of ONE home 300 slots before the array's end: a chain that wraps, in src and -- the same hashes have the same home in a
    table of the same size -- in minus; beside them keys spread over homes in the middle"""
    s = 16
    rng = random.Random(4100 + k)
    n = 1 << s
    _, kms = craft(k, s, n - 300, 1000, rng)
    assert 1000 > MAXPROBE // 2 and 1000 - 300 > 0, "the chain wraps"
    _, more = craft_edge(k, s, n // 2, 64, 400, rng)
    _, extra = craft_edge(k, s, n // 4, 16, 50, rng)
    sd = {km: 1 + i % 5 for i, km in enumerate(kms + more)}
    md = mixed_minus(kms + more, sd, extra)
    src, minus = filled(KT, k, s, sd), filled(KT, k, s, md)
    want, counters, missing = check_subtract(KT, src, minus, sd, md)
    assert counters[1] > 400 and counters[2] > 100 and counters[3] > 10 and counters[4] > 400 and missing == 50, "vacuous case"
    assert any(c < sd[km] for km, c in want.items()) and any(c == sd[km] for km, c in want.items())
    close(src, minus)


@pytest.mark.parametrize("k", [21, 41])
def test_keys_on_both_sides_of_a_piece_edge(KT, k):
    """JASPER_SUBTRACT_PIECE=4096 on a table of 2^16 slots: 16 pieces.  A chain of 900 keys starts 450 slots before a piece's end, one
    before the array's, and clusters sit on the last and first homes of other pieces: every key is met once, by the piece its SLOT
    lies in"""
    s, piece = 16, 4096
    rng = random.Random(4200 + k)
    n = 1 << s
    kms = []
    for home in (3 * piece - 450, n - 450):
        kms += craft(k, s, home, 900, rng)[1]
    for edge in (piece, 7 * piece, 12 * piece):
        kms += craft_edge(k, s, edge - 8, 16, 160, rng)[1]
    kms = list(dict.fromkeys(kms))
    sd = {km: 1 + i % 7 for i, km in enumerate(kms)}
    md = mixed_minus(kms, sd)
    src, minus = filled(KT, k, s, sd), filled(KT, k, s, md)
    whole = check_subtract(KT, src, minus, sd, md)
    with env(JASPER_SUBTRACT_PIECE=str(piece)):
        assert check_subtract(KT, src, minus, sd, md) == whole
    with env(JASPER_SUBTRACT_PIECE="4097"):                                               # a piece that is no multiple of a wave or a workgroup
        assert check_subtract(KT, src, minus, sd, md) == whole
    assert min(whole[1]) > 10
    for bad in ("0", "x", str((1 << 24) + 1), ""):
        with env(JASPER_SUBTRACT_PIECE=bad):
            with pytest.raises(Exception, match="JASPER_SUBTRACT_PIECE must be a number of slots"):
                KT.subtract(src, minus)
    close(src, minus)


@pytest.mark.parametrize("k", [21, 41])
@pytest.mark.parametrize("s_src,s_minus", [(16, 18), (18, 16)])
def test_tables_of_different_sizes(KT, k, s_src, s_minus):
    """src of 2^16 slots against minus of 2^18 and the reverse: a key's home and tag differ between the two (k = 41: 2^16 slots keep
    the low remainder bits in the ext word, 2^18 too; k = 21: both narrow)"""
    rng = random.Random(4300 + k + s_src)
    _, kms = craft_edge(k, s_src, (1 << s_src) - 8, 24, 600, rng)
    _, extra = craft_edge(k, s_minus, 1000, 10, 40, rng)
    extra = [km for km in extra if km not in set(kms)]
    sd = {km: 2 + i % 4 for i, km in enumerate(kms)}
    md = mixed_minus(kms, sd, extra)
    src, minus = filled(KT, k, s_src, sd), filled(KT, k, s_minus, md)
    _, counters, missing = check_subtract(KT, src, minus, sd, md)
    assert counters[1] > 200 and counters[2] > 50 and counters[3] > 5 and missing == len(extra) > 0
    close(src, minus)


def test_counts_beyond_32_bits_and_every_class(KT):
    """2^33 + 5 minus 7 stays above 32 bits; equal counts drop the key; 1 - 0 keeps it; minus larger than src is an underflow and the
    key is absent; a minus key src lacks is missing.  A lookup's 32-bit clamp would make 2^33 + 5 and 2^32 + 1 equal"""
    k, s = 31, 16
    rng = random.Random(4401)
    _, kms = craft_edge(k, s, 77, 8, 40, rng)
    _, extra = craft_edge(k, s, 30000, 4, 6, rng)
    sd = {km: 1 for km in kms}
    md = {}
    sd[kms[0]], md[kms[0]] = 2**33 + 5, 7
    sd[kms[1]], md[kms[1]] = 9, 9
    sd[kms[3]], md[kms[3]] = 3, 4
    sd[kms[4]], md[kms[4]] = 2**33 + 5, 2**32 + 1
    sd[kms[5]], md[kms[5]] = 2**40, 2**40
    sd[kms[6]], md[kms[6]] = 2**32 + 1, 2**33 + 5
    sd[kms[7]], md[kms[7]] = 2**63 + 9, 2**63 + 1
    md.update({km: 1 for km in extra})
    src, minus = filled(KT, k, s, sd), filled(KT, k, s, md)
    want, counters, missing = check_subtract(KT, src, minus, sd, md)
    assert want[kms[0]] == 2**33 - 2 and kms[1] not in want and want[kms[2]] == 1 and kms[3] not in want
    assert want[kms[4]] == 2**32 + 4 and kms[5] not in want and kms[6] not in want and want[kms[7]] == 8
    assert counters == (40, 7, 2, 2, 36) and missing == 6
    close(src, minus)


@pytest.mark.parametrize("k", [21, 41])
def test_empty_minus_and_empty_source(KT, k):
    s = 16
    rng = random.Random(4500 + k)
    _, kms = craft_edge(k, s, 100, 50, 500, rng)
    sd = {km: 2 + i % 3 for i, km in enumerate(kms)}
    src, empty = filled(KT, k, s, sd), filled(KT, k, s, {})
    want, counters, missing = check_subtract(KT, src, empty, sd, {})
    assert want == sd and counters == (500, 0, 0, 0, 500) and missing == 0
    want, counters, missing = check_subtract(KT, empty, src, {}, sd)
    assert want == {} and counters == (0, 0, 0, 0, 0) and missing == 500
    close(src, empty)


def test_refusals(KT):
    import ctypes as C
    from jasper_amd.table import check
    k, s = 21, 16
    rng = random.Random(4601)
    _, kms = craft_edge(k, s, 5, 10, 60, rng)
    sd, md = {km: 2 for km in kms}, {km: 1 for km in kms[0::2]}
    src, minus, other_k = filled(KT, k, s, sd), filled(KT, k, s, md), KT(k + 2, min_slots=1 << s)
    with pytest.raises(Exception, match="source table and the minus table are the same table"):
        KT.subtract(src, src)
    with pytest.raises(Exception, match="different k"):
        KT.subtract(src, other_k)
    with pytest.raises(TypeError, match="minus table must be an open KmerTable"):
        KT.subtract(src, None)

    def raw(dst, a, b):
        out, secs = (C.c_uint64 * 5)(), C.c_double(0)
        check(src._L.jasper_table_subtract(dst._h, a._h, b._h, out, C.byref(secs)))
        return tuple(out)

    full = filled(KT, k, s, {kms[0]: 1})
    with pytest.raises(Exception, match="destination table must be empty"):
        raw(full, src, minus)
    with pytest.raises(Exception, match="source table and the destination table are the same table"):
        raw(src, src, minus)
    with pytest.raises(Exception, match="minus table and the destination table are the same table"):
        raw(minus, src, minus)
    with pytest.raises(Exception, match="different k"):
        raw(other_k, src, minus)
    assert lu.table_dict(full) == {kms[0]: 1} and lu.table_dict(src) == sd and lu.table_dict(minus) == md      # nothing was touched
    full.clear()
    assert raw(full, src, minus) == restate(sd, md)[1]
    assert lu.table_dict(full) == restate(sd, md)[0]
    close(src, minus, other_k, full)
