"""CPU: the helpers of test_gpu_table_layout.py (tests/layout_util.py) -- the restated hash against the library's inverse, what
`craft` promises, the part-of-key function and the pigeonhole facts the GPU scenarios rely on.  Host arithmetic only (the
library's jasper_debug_mix hook): no GPU involved."""
import ctypes as C
import random

import pytest

import layout_util as lu
from layout_util import MAXPROBE, craft, craft_edge, decode, py_mix

KS = (17, 25, 31, 32, 33, 37, 45, 64)


@pytest.mark.parametrize("k", KS)
def test_decode_inverts_the_restated_mix(k):
    from jasper_amd import _lib
    L = _lib.lib()
    rng = random.Random(k)
    B = 2 * k
    out = (C.c_uint64 * 2)()
    for x in [0, 1, (1 << B) - 1, 1 << (B - 1)] + [rng.getrandbits(B) for _ in range(300)]:
        h = py_mix(x, B)
        assert 0 <= h < (1 << B)
        assert decode(k, h) == lu.kmer_of_int(x, k)
        assert L.jasper_debug_mix(k, 0, x >> 64, x & lu.M64, out) == 0 and ((out[0] << 64) | out[1]) == h   # the forward hook agrees too
    km = "ACGT" * 16
    assert lu.kmer_of_int(lu.int_of_kmer(km[:k]), k) == km[:k] and lu.revcomp("AACG") == "CGTT" and lu.canon("TTTT") == "AAAA"


@pytest.mark.parametrize("k,s", [(17, 16), (31, 16), (32, 20), (37, 22), (37, 16), (45, 16), (64, 16), (31, 40)])
def test_craft_places_keys(k, s):
    rng = random.Random(7 * k + s)
    home = rng.randrange(1 << s)
    hs, kms = craft(k, s, home, 200, rng)
    assert len(set(hs)) == 200 and all(h >> (2 * k - s) == home for h in hs)
    for h, km in zip(hs, kms):
        assert len(km) == k and km <= lu.revcomp(km) and lu.hash_of_kmer(km) == h and py_mix(lu.int_of_kmer(km), 2 * k) == h
    # about half of all hashes of a home are canonical k-mers (what the cap of 8 n candidates rests on)
    alls = craft(k, s, home, 400, rng, canonical=False)[0]
    share = sum(decode(k, h) <= lu.revcomp(decode(k, h)) for h in alls) / 400
    assert 0.4 < share < 0.6
    # given remainders: taken in order, only the canonical ones
    rems = [rng.getrandbits(2 * k - s) for _ in range(50)]
    got = craft(k, s, home, None, rng, rem=rems)[0]
    assert got == [h for h in ((home << (2 * k - s)) | r for r in rems) if decode(k, h) <= lu.revcomp(decode(k, h))]
    with pytest.raises(AssertionError):
        craft(k, s, home, 3, rng, rem=lambda r: 5)          # one remainder cannot give three keys: the cap of 8 n candidates


def test_split_and_join():
    rng = random.Random(3)
    for k, s in [(31, 16), (37, 22), (37, 16), (45, 16), (64, 16), (64, 11)]:
        for _ in range(50):
            h = rng.getrandbits(2 * k)
            home, tag_rem, ext = lu.split(k, s, h)
            assert lu.join(k, s, home, tag_rem, ext) == h
            assert (ext is not None) == (2 * k - s > 53) and tag_rem < (1 << 53) and home < (1 << s)


def test_part_of_key():
    for nparts in (1, 2, 3, 7, 8):
        for k in (17, 31, 37, 64):
            B = 2 * k
            assert lu.part_of(k, 0, nparts) == 0 and lu.part_of(k, (1 << B) - 1, nparts) == nparts - 1
            for p in range(1, nparts):
                t = -((-p << 32) // nparts)                      # ceil(p 2^32 / nparts): the first top-32 value of partition p
                assert lu.part_of(k, t << (B - 32), nparts) == p and lu.part_of(k, (t << (B - 32)) - 1, nparts) == p - 1
    assert lu.part_of(8, 0xFFFF, 4) == 3 and lu.part_of(8, 0x4000, 4) == 1          # 2k < 32: the hash is the TOP of the 32 bits
    s = 20
    for nparts in (2, 3, 7, 8):
        for p in range(nparts):
            home = lu.last_home_of_part(s, p, nparts)
            assert ((home << 12) * nparts) >> 32 == p
            assert p == nparts - 1 and home == (1 << s) - 1 or (((home + 1) << 12) * nparts) >> 32 == p + 1
            # a full chain of 1024 keys on that home lies in the NEXT partition's home range (the last one wraps to slot 0)
            assert home + 1023 >= (1 << s) if p == nparts - 1 else lu.last_home_of_part(s, p + 1, nparts) > home + 1023


def test_pigeonhole_facts_of_the_scenarios():
    rng = random.Random(11)
    # longest chain: 1024 keys of one home fill probe offsets 0 .. 1023 and nothing else; one more has nowhere to go
    k, s = 31, 16
    hs, _ = craft(k, s, (1 << s) - 1, MAXPROBE + 1, rng)
    assert len({h >> (2 * k - s) for h in hs}) == 1 and len(set(hs)) == MAXPROBE + 1 > MAXPROBE
    # the cluster growth cannot split: the top 40 bits are shared, so the home is shared in every table of up to 2^40 slots
    hs, _ = craft(31, 40, rng.getrandbits(40), 1100, rng)
    assert all(len({h >> (62 - s2) for h in hs}) == 1 for s2 in range(16, 25)) and len(hs) > MAXPROBE
    # region-wise import: 80 keys homed in the last 16 slots of a 4096-slot region -- at least 64 cannot stay in the region
    for k, s in [(31, 16), (37, 22)]:
        for reg in (3, (1 << (s - 12)) - 1):
            hs, _ = craft_edge(k, s, (reg + 1) * 4096 - 16, 16, 80, rng)
            homes = [h >> (2 * k - s) for h in hs]
            assert len(hs) == 80 and all(h >> 12 == reg and (h & 4095) >= 4080 for h in homes)
    # counting: regions of 2^12 slots (2^11 in a wide table)
    for k, s, rbits in [(37, 24, 12), (51, 24, 11)]:
        g = lu.region_edge_keys(k, s, rbits, rng)
        R = 1 << rbits
        home = lambda h: h >> (2 * k - s)
        for name in ("edge", "last", "blocked"):
            homes = [home(h) for h in g[name][0]]
            assert len(homes) == 64 and len({h >> rbits for h in homes}) == 1 and all(h % R >= R - 16 for h in homes)      # 64 keys, 16 slots
        assert {home(h) >> rbits for h in g["last"][0]} == {(1 << (s - rbits)) - 1}
        blocked = home(g["blocked"][0][0]) >> rbits
        assert sorted(home(h) for h in g["blockers"][0]) == [(blocked + 1) * R + i for i in range(32)]
        ch = {home(h) for h in g["chain"][0]}
        assert len(ch) == 1 and len(g["chain"][0]) == 600 and min(ch) % R + 600 > R
        allk = [km for v in g.values() for km in v[1]]
        assert len(set(allk)) == len(allk)


def test_reference_counts_strings():
    k = 5
    r = lu.Ref(k).add_bases("ACGTACGTNNACGTAacgta")
    want = {}
    for piece in ("ACGTACGT", "ACGTAACGTA"):
        for i in range(len(piece) - k + 1):
            km = lu.canon(piece[i:i + k])
            want[km] = want.get(km, 0) + 1
    assert dict(r.c) == want and r.occurrences == sum(want.values()) and r.distinct == len(want)
    r.add_kmers(["AAAAA", "AAAAC"], [2**32 + 5, 10001])
    assert r.lookup(["AAAAA", "TTTTT", "GTTTT", "CCCCC"]) == [2**32 - 1, 2**32 - 1, 10001, 0]
    h = r.histogram()
    assert h[10001] == 2 and sum(h) == r.distinct and h[0] == 0
    assert r.clamped().c["AAAAA"] == 2**32 - 1
    assert lu.unpack(37, *lu.pack(37, 5 << 64 | 9, 2**54 - 1)) == (5 << 64 | 9, 2**54 - 1) and lu.unpack(31, *lu.pack(31, 77, 2**63)) == (77, 2**63)
    with pytest.raises(AssertionError):
        lu.pack(37, 1, 2**54)
    counts, runs = lu.Ref(3).add_kmers(["AAA", "AAC"], [5, 1]).report(["AAACNAAA", "aaa"], 2)
    assert counts == [(6, 3, 1, 0), (1, 1, 0, 0)] and runs == [(0, 1, 1, 0, 1)]
