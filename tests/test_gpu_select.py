"""GPU: KmerTable.select (jasper_table_select, csrc/select.hip) against tests/markers_ref.select, fed by Python dicts of canonical k-mer
strings.  The tables are filled with keys placed by chosen hash (tests/layout_util.py: craft, entries, import_entries), so a test decides
which slots, chains and piece edges the sweep meets; nothing expected here comes from the code under test.

Compared, bit-exact: the destination's exported entries (key -> src's 64-bit count), the four counters, info()["distinct"], lookup() of
the selected keys (their clamped counts) and of the dropped ones (0)."""
import os
import random

import pytest

import layout_util as lu
import markers_ref as mr
from layout_util import MAXPROBE, U32, craft, craft_edge, entries

pytestmark = pytest.mark.gpu

# the select kernel's sweep (csrc/select.hip, csrc/spectra.hpp): at most 256 * 8 workgroups of SP_THREADS = 256 threads, SP_BATCH = 4
# slots a thread and trip -- a piece with more slots than this takes more than one trip of the kernel's loop
SWEEP_SLOTS = 256 * 8 * 256 * 4
PIECE = 1 << 24          # csrc/select.hpp: SEL_PIECE


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


def check_select(KT, src, absent, solid, sd, ad, rd, thre_src=1, thre_solid=1):
    want, counters = mr.select(sd, ad, rd, thre_src, thre_solid)
    dst, st = KT.select(src, absent, solid, thre_src, thre_solid)
    try:
        got = lu.table_dict(dst)
        assert got == want, lu._diff(got, want)
        assert (st["candidates"], st["in_absent"], st["not_solid"], st["selected"]) == counters
        assert dst.info()["distinct"] == len(want) and dst.k == src.k
        assert st["seconds"] > 0
        keys = list(want)[:2000]
        assert dst.lookup(keys) == [min(want[km], U32) for km in keys]
        dropped = [km for km in sd if km not in want][:2000] + [km for km in ad if km not in want][:500]
        assert dst.lookup(dropped) == [0] * len(dropped)
    finally:
        dst.close()
    # the sources are what they were
    assert src.info()["distinct"] == len(sd) and absent.info()["distinct"] == len(ad)
    return want, counters


def close(*tables):
    for t in tables:
        if t is not None:
            t.close()


# ---- 1. a full probe chain that wraps, in all three tables -----------------------------------------------------------------------------
def test_chain_at_the_end_of_the_array_k21(KT):
    """1000 keys of ONE home 300 slots before the array's end: a chain that wraps, in src and -- the same hashes have the same home in a
    table of the same size -- for the keys they hold, in absent and in solid too; beside them keys spread over homes in the middle
    (well clear of the 700 slots the chain takes at the array's start: a key homed there would be pushed past its last probe)"""
    k, s = 21, 16
    rng = random.Random(2101)
    n = 1 << s
    hs, kms = craft(k, s, n - 300, 1000, rng)
    assert 1000 > MAXPROBE // 2 and 1000 - 300 > 0, "the chain wraps"
    _, more = craft_edge(k, s, n // 2, 64, 400, rng)
    sd = {km: 1 + i % 5 for i, km in enumerate(kms + more)}
    ad = {km: 3 for km in (kms + more)[0::3]}
    rd = {km: (2 if i % 2 else 1) for i, km in enumerate((kms + more)[1::3])}          # half of them solid at threshold 2
    rd.update({km: 9 for km in (kms + more)[0::6]})                                    # (solid AND in absent: in_absent wins)
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s, rd)
    want, counters = check_select(KT, src, absent, solid, sd, ad, rd, 1, 2)
    assert counters[1] > 400 and counters[2] > 400 and counters[3] > 100, "vacuous case"
    check_select(KT, src, absent, None, sd, ad, None)
    close(src, absent, solid)


# ---- 2. mixed geometry: wide src and absent, narrow solid ----------------------------------------------------------------------------------
def test_wide_source_and_narrow_solid_k37(KT):
    """src and absent have 2^16 slots (k = 37: the low 64 remainder bits in the ext word), solid 2^22 (the whole remainder in the tag).
    absent holds keys that share home AND tag remainder with selected keys of src and differ in the ext word alone: a probe that
    compared tags only would drop them"""
    k, s, s_solid = 37, 16, 22
    assert lu.is_wide(k, s) and not lu.is_wide(k, s_solid)
    rng = random.Random(3716)
    hs, kms = craft_edge(k, s, (1 << s) - 8, 24, 300, rng)                              # homes across the array's end
    near = lu.absent_neighbours(k, s, hs[:40], set(kms), rng)
    assert len(near) >= 80
    sd = {km: 1 + i % 4 for i, km in enumerate(kms)}
    sd.update({km: 6 for km in near[0::4]})                                              # (some neighbours are src's too, and dropped: absent holds them)
    ad = dict({km: 2 for km in near}, **{km: 1 for km in kms[0::7]})
    rd = dict({km: 3 for km in kms[0::2]}, **{km: 3 for km in near})
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s_solid, rd)
    want, counters = check_select(KT, src, absent, solid, sd, ad, rd, 1, 3)
    assert all(km in want for km in kms[:40:2] if km not in ad), "the keys whose neighbours absent holds are selected"
    assert counters[1] >= len(near[0::4]) + 40 and counters[2] > 100 and counters[3] > 100
    check_select(KT, src, absent, None, sd, ad, None)
    close(src, absent, solid)


# ---- 3. k = 63 -------------------------------------------------------------------------------------------------------------------
def test_k63(KT):
    k, s = 63, 16
    rng = random.Random(6316)
    _, kms = craft_edge(k, s, 12345, 200, 600, rng)
    near = lu.absent_neighbours(k, s, [lu.hash_of_kmer(km) for km in kms[:10]], set(kms), rng)
    sd = {km: 1 + i % 3 for i, km in enumerate(kms)}
    ad = dict({km: 1 for km in kms[0::4]}, **{km: 1 for km in near})
    rd = {km: 1 + i % 2 for i, km in enumerate(kms[0::3])}
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s + 1, rd)
    _, counters = check_select(KT, src, absent, solid, sd, ad, rd, 1, 2)
    assert min(counters) > 50
    check_select(KT, src, absent, solid, sd, ad, rd, 2, 1)
    close(src, absent, solid)


# ---- 4. counts beyond 32 bits --------------------------------------------------------------------------------------------------------
def test_counts_beyond_32_bits(KT):
    """solid's count is clamped to 2^32-1 before it meets the threshold: 2^32 + 5 meets 2^32 - 1, 2^32 - 2 does not.  src's count is
    compared and handed on whole"""
    k, s = 31, 16
    rng = random.Random(3101)
    _, kms = craft_edge(k, s, 77, 8, 40, rng)
    sd = {km: 1 + i for i, km in enumerate(kms)}
    sd[kms[0]], sd[kms[1]], sd[kms[2]] = 2**32 + 7, 2**40 + 3, 2**63 + 1
    rd = {km: 2**32 + 5 for km in kms[0:20]}
    rd[kms[3]], rd[kms[4]], rd[kms[5]] = 2**32 - 2, 2**32 - 1, 2**50
    ad = {kms[19]: 2**33}
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s, rd)
    want, counters = check_select(KT, src, absent, solid, sd, ad, rd, 1, U32)
    assert counters == (40, 1, 21, 18) and want[kms[0]] == 2**32 + 7 and want[kms[1]] == 2**40 + 3 and want[kms[2]] == 2**63 + 1
    assert kms[3] not in want and kms[4] in want and kms[5] in want
    want, counters = check_select(KT, src, absent, None, sd, ad, None, U32, 1)           # the largest threshold: 2^32-1
    assert set(want) == {kms[0], kms[1], kms[2]}
    close(src, absent, solid)


# ---- 5. the source threshold ------------------------------------------------------------------------------------------------------------
def test_source_threshold_of_3(KT):
    k, s = 25, 16
    rng = random.Random(2503)
    _, kms = craft_edge(k, s, 40000, 300, 900, rng)
    sd = {km: 1 + i % 5 for i, km in enumerate(kms)}
    ad = {km: 1 for km in kms[0::4]}
    rd = {km: 1 + i % 3 for i, km in enumerate(kms[0::2])}
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s, rd)
    want, counters = check_select(KT, src, absent, solid, sd, ad, rd, 3, 2)
    assert counters[0] == sum(1 for c in sd.values() if c >= 3) < len(sd) and min(want.values()) >= 3 and min(counters) > 50
    close(src, absent, solid)


# ---- 6. degenerate results --------------------------------------------------------------------------------------------------------------
def test_empty_absent_and_absent_equal_to_source(KT):
    k, s = 21, 16
    rng = random.Random(2106)
    _, kms = craft_edge(k, s, 100, 50, 500, rng)
    sd = {km: 2 + i % 3 for i, km in enumerate(kms)}
    src, empty, same = filled(KT, k, s, sd), filled(KT, k, s, {}), filled(KT, k, s, dict.fromkeys(sd, 1))
    want, counters = check_select(KT, src, empty, None, sd, {}, None)
    assert want == sd and counters == (500, 0, 0, 500)
    want, counters = check_select(KT, src, same, None, sd, dict.fromkeys(sd, 1), None)
    assert want == {} and counters == (500, 500, 0, 0)
    want, counters = check_select(KT, empty, src, same, {}, sd, dict.fromkeys(sd, 1))
    assert want == {} and counters == (0, 0, 0, 0)
    close(src, empty, same)


# ---- 7. pieces and sweeps ------------------------------------------------------------------------------------------------------------------
def test_sixteen_pieces_with_chains_across_their_edges(KT):
    """JASPER_SELECT_PIECE=4096 on a table of 2^16 slots: 16 pieces.  Two chains of 900 keys start 450 slots before a piece's end, one of
    them before the array's, and clusters sit on the last and first homes of other pieces: every key is met once, by the piece its
    SLOT lies in"""
    k, s, piece = 21, 16, 4096
    rng = random.Random(2107)
    n = 1 << s
    kms = []
    for home in (3 * piece - 450, n - 450):
        kms += craft(k, s, home, 900, rng)[1]
    for edge in (piece, 7 * piece, 12 * piece):
        kms += craft_edge(k, s, edge - 8, 16, 160, rng)[1]
    kms = list(dict.fromkeys(kms))
    sd = {km: 1 + i % 7 for i, km in enumerate(kms)}
    ad = {km: 1 for km in kms[0::3]}
    rd = {km: 1 + i % 2 for i, km in enumerate(kms[1::3] + kms[2::9])}
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, s, ad), filled(KT, k, s, rd)
    whole = check_select(KT, src, absent, solid, sd, ad, rd, 2, 2)
    with env(JASPER_SELECT_PIECE=str(piece)):
        cut = check_select(KT, src, absent, solid, sd, ad, rd, 2, 2)
    assert cut == whole and min(whole[1]) > 100
    for p in ("4097", "65535"):                                                          # pieces that are no multiple of a wave, a workgroup or a trip
        with env(JASPER_SELECT_PIECE=p):
            assert check_select(KT, src, absent, None, sd, ad, None) == (mr.select(sd, ad, None, 1, 1))
    for bad in ("0", "x", str(PIECE + 1), ""):
        with env(JASPER_SELECT_PIECE=bad):
            with pytest.raises(Exception, match="JASPER_SELECT_PIECE must be a number of slots"):
                KT.select(src, absent)
    close(src, absent, solid)


def test_a_table_larger_than_one_sweep_of_the_grid(KT):
    """2^22 slots in one piece: the kernel's grid covers SWEEP_SLOTS = 2^21 slots a trip, so its loop makes a second trip; keys on the
    last homes of the first trip, the first of the second and the array's end"""
    k, s = 31, 22
    n = 1 << s
    assert SWEEP_SLOTS < n <= PIECE and not lu.is_wide(k, s)
    rng = random.Random(3122)
    kms = []
    for first in (0, SWEEP_SLOTS - 40, SWEEP_SLOTS + 100000, n - 40):
        kms += craft_edge(k, s, first, 80, 240, rng)[1]
    sd = {km: 1 + i % 3 for i, km in enumerate(kms)}
    ad = {km: 1 for km in kms[0::5]}
    rd = {km: 2 for km in kms[0::2]}
    src, absent, solid = filled(KT, k, s, sd), filled(KT, k, 16, ad), filled(KT, k, 20, rd)
    whole = check_select(KT, src, absent, solid, sd, ad, rd, 1, 2)
    assert min(whole[1]) > 100
    with env(JASPER_SELECT_PIECE=str(SWEEP_SLOTS + 4096)):                                # two pieces, the first with a second trip of 4096 slots
        assert check_select(KT, src, absent, solid, sd, ad, rd, 1, 2) == whole
    close(src, absent, solid)


# ---- 8. the census counts what the select keeps --------------------------------------------------------------------------------------------
def small_trio(KT, seed):
    """a trio's three counted tables (test_gpu_hapmers.Trio) and their dicts keyed by k-mer string"""
    from test_gpu_hapmers import TILE, Trio
    from test_gpu_hapmer_census import trio_dicts
    t = Trio(KT, seed, 25, TILE // 2)
    return t, [dict((km.decode(), c) for km, c in d.items()) for d in trio_dicts(t)]


def test_selected_equals_the_census(KT):
    from test_gpu_hapmers import THRE
    t, (md, pd, cd) = small_trio(KT, 4200)
    for child, cdict in ((t.R, cd), (None, None)):
        for a, b, ad_, bd_ in ((t.M, t.P, md, pd), (t.P, t.M, pd, md)):
            want, counters = check_select(KT, a, b, child, ad_, bd_, cdict, THRE, THRE)
            cen = KT.hapmer_census_parents(a, b, None, THRE, THRE, THRE, _child=child)
            assert cen.mat[0] == counters[3] == len(want) > 100
    t.close()


def test_an_attached_solid_table_is_read_through_its_shards(KT):
    from test_gpu_hapmers import THRE
    from test_gpu_shard import make_shards
    t, (md, pd, cd) = small_trio(KT, 4201)
    shards, _ = make_shards(KT, t.R, 2, t.R.info()["slots"])
    for o, sh in enumerate(shards):
        sh.attach_tables(shards, o)
    whole = mr.select(md, pd, cd, THRE, THRE)
    for sh in shards:
        dst, st = KT.select(t.M, t.P, sh, THRE, THRE)
        assert lu.table_dict(dst) == whole[0] and (st["candidates"], st["in_absent"], st["not_solid"], st["selected"]) == whole[1]
        dst.close()
    with pytest.raises(Exception, match="source table must be a whole table"):
        KT.select(shards[0], t.P)
    with pytest.raises(Exception, match="absent table must be a whole table"):
        KT.select(t.M, shards[1])
    close(*shards)
    t.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(KT):
    import ctypes as C
    from jasper_amd.table import check
    k, s = 21, 16
    rng = random.Random(2109)
    _, kms = craft_edge(k, s, 5, 10, 60, rng)
    sd, ad = {km: 2 for km in kms}, {km: 1 for km in kms[0::2]}
    src, absent, other_k = filled(KT, k, s, sd), filled(KT, k, s, ad), KT(k + 2, min_slots=1 << s)
    with pytest.raises(Exception, match="source table and the absent table are the same table"):
        KT.select(src, src)
    with pytest.raises(Exception, match="absent table and the solid table are the same table"):
        KT.select(src, absent, absent)
    with pytest.raises(Exception, match="source table and the solid table are the same table"):
        KT.select(src, absent, src)
    with pytest.raises(Exception, match="different k"):
        KT.select(src, other_k)
    with pytest.raises(Exception, match="different k"):
        KT.select(src, absent, other_k)
    with pytest.raises(Exception, match="source threshold must be at least 1"):
        KT.select(src, absent, None, 0, 1)
    with pytest.raises(Exception, match="solid threshold must be at least 1"):
        KT.select(src, absent, None, 1, 0)
    with pytest.raises(TypeError, match="absent table must be an open KmerTable"):
        KT.select(src, None)

    def raw(dst, a, b):
        out, secs = (C.c_uint64 * 4)(), C.c_double(0)
        check(src._L.jasper_table_select(dst._h, a._h, b._h, None, 1, 1, out, C.byref(secs)))
        return tuple(out)

    full = filled(KT, k, s, {kms[0]: 1})
    with pytest.raises(Exception, match="destination table must be empty"):
        raw(full, src, absent)
    with pytest.raises(Exception, match="source table and the destination table are the same table"):
        raw(src, src, absent)
    with pytest.raises(Exception, match="absent table and the destination table are the same table"):
        raw(absent, src, absent)
    with pytest.raises(Exception, match="different k"):
        raw(other_k, src, absent)
    assert lu.table_dict(full) == {kms[0]: 1} and lu.table_dict(src) == sd and lu.table_dict(absent) == ad      # nothing was touched
    # a cleared table is an empty one
    full.clear()
    assert raw(full, src, absent) == mr.select(sd, ad, None, 1, 1)[1]
    assert lu.table_dict(full) == mr.select(sd, ad, None, 1, 1)[0]
    close(src, absent, other_k, full)
