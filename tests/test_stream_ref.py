"""CPU: the whole-stream reference of tests/test_gpu_count_text.py (stream_ref.py) against the string Counter of layout_util, its
additivity over cuts, and the planted texts at a small scale."""
import random

import numpy as np
import pytest

import layout_util as lu
import stream_ref as sr

KS = [16, 32, 33, 37, 38, 48, 49, 64]          # the k of test_gpu_count_text.py
MORE_KS = [1, 2, 15, 21, 31, 63]


def _texts(k):
    rng = random.Random(900 + k)
    mixed = "".join(rng.choice("ACGTacgtN") if rng.random() < 0.04 else rng.choice("ACGT") for _ in range(4000))
    every = bytearray(rng.choice(b"ACGT") for _ in range(5000))
    for i, v in enumerate(range(256)):                                       # every byte value, at distances around k
        every[100 + i * (k // 3 + 7) % 4800] = v
    every[-1] = ord("n")
    stretches = "".join("".join(rng.choice("ACGTacgt") for _ in range(n)) + sep
                        for n, sep in ((1500, "N"), (k, "\n"), (k - 1, "N"), (2200, "\x00"), (k + 1, ">"), (900, "")))
    repeat = ("ACGTTGCA" * 40 + "A" * 200 + "AC" * 150)                    # palindromes, runs: keys with large counts
    short = "ACGTACGTAC" * 7
    return [mixed, bytes(every), stretches, repeat, short[:k - 1], short[:k] if k <= 64 else "", "", "N" * (2 * k)]


@pytest.mark.parametrize("k", KS + MORE_KS)
def test_count_stream_equals_the_string_counter(k):
    for text in _texts(k):
        want = sr.from_counter(lu.kmer_counter(text, k), k)
        got = sr.count_stream(text, k)
        assert all(a.dtype == np.uint64 for a in got)
        assert sr.same(got, want), (k, len(text))
        assert int(got[2].sum()) == int(sr.valid_windows(text, k).sum())
        order = np.lexsort((got[1], got[0]))
        assert np.array_equal(order, np.arange(order.size)), "sorted by (hi, lo)"
        # lookups and the histogram read the same counts
        for km, c in list(lu.kmer_counter(text, k).items())[:20]:
            assert sr.lookup(got, lu.hash_of_kmer(lu.revcomp(km))) == c
        h = [0] * lu.HISTO_BINS
        for c in lu.kmer_counter(text, k).values():
            h[min(c, 10001)] += 1
        assert sr.histogram(got) == h


@pytest.mark.parametrize("k", KS)
def test_counts_add_over_a_cut_with_k_minus_1_bases_of_overlap(k):
    for text in _texts(k)[:4]:
        b = sr.as_array(text)
        whole = sr.count_stream(b, k)
        for a in (0, 1, k - 2, k - 1, k, k + 1, 1000, 1024, b.size - k, b.size - 1, b.size):
            if not 0 <= a <= b.size:
                continue
            parts = sr.add(sr.count_stream(b[:a], k), sr.count_stream(b[max(0, a - k + 1):], k))
            assert sr.same(parts, whole), (k, a)
        assert sr.same(sr.add(whole, whole), sr.times(whole, 2))
        empty = sr.count_stream(b"", k)
        assert sr.same(sr.add(whole, empty), whole)


def test_tile_records_count_windows_by_their_last_base():
    k, tile = 21, 64
    t = sr.seam_text(sr.base_text(64 * 9 + 5, 1009), k, tile)[0]
    both, h0, h1 = sr.tile_records(t, k, tile)
    v = sr.valid_windows(t, k)
    want = [[0, 0] for _ in range(10)]
    for i in np.flatnonzero(v):
        e = i + k - 1
        want[e // tile][(e % 16) // 8] += 1
    assert [list(x) for x in zip(h0, h1)] == want and list(both) == [a + b for a, b in want]


TILE, PERIOD, NT = 64, 1009, 700


@pytest.mark.parametrize("k", KS)
def test_planted_texts_hold_what_their_builder_claims(k):
    n = TILE * NT + 5
    base = sr.base_text(n, PERIOD)
    assert base.size == n and set(base.tolist()) == set(b"ACGT")
    assert np.array_equal(base[:PERIOD], base[PERIOD:2 * PERIOD]) and np.array_equal(base[:n - 3 * PERIOD], base[3 * PERIOD:])
    # seams
    text, plants = sr.seam_text(base, k, TILE)
    bo, ao = sr.before_offsets(k), sr.after_offsets(k)
    assert len(bo) == 10 and len(ao) == 7
    at = {p: v for p, v, _, _ in plants}
    assert len(at) == len(plants)
    code = sr._CODE[text]
    assert sorted(np.flatnonzero(code == 255).tolist()) == sorted(at), "the invalid bytes are exactly the plants"
    for p, v, T, off in plants:
        assert text[p] == v and v in sr.INVALID_BYTES and p == T * TILE + off
        assert off in (bo[(T - 1) % 10], ao[(T - 1) % 7])
    # every boundary has its two plants unless one fell on another's position or outside the text
    claimed = {p: (T, off) for p, _, T, off in plants}
    for T in range(1, NT + 1):
        for off in (bo[(T - 1) % 10], ao[(T - 1) % 7]):
            p = T * TILE + off
            assert not 0 <= p < n or claimed[p] == (T, off) or claimed[p][0] > T, "only a later boundary's plant takes a position"
    assert len(plants) >= 2 * NT - NT // 4
    values = [v for _, v, _, _ in plants]
    assert set(values) == set(sr.INVALID_BYTES) and min(values.count(v) for v in sr.INVALID_BYTES) >= 2
    keep = code != 255
    assert np.array_equal(text[keep] & 0xDF, base[keep]), "the other bytes are the base text's, in either case"
    low = float(np.mean(text[keep] != base[keep]))
    assert 0.02 < low < 0.04, low
    # a longer text's prefix is the shorter text, but for plants that lie past the shorter text's end
    longer, _ = sr.seam_text(sr.base_text(n + 7 * TILE + 3, PERIOD), k, TILE)
    assert np.array_equal(longer[:n - 70], text[:n - 70])
    # runs
    rt, runs = sr.run_text(base, TILE, 20, 50, extra=20, lead=10)
    (sa, la), (sc, lc) = runs
    assert (sa, la, sc, lc) == (20 * TILE - 10, TILE + 20, 50 * TILE - 10, TILE + 20)
    assert bytes(rt[sa:sa + la]) == b"A" * la and bytes(rt[sc:sc + lc]) == b"AC" * (lc // 2)
    other = np.ones(n, dtype=bool)
    other[sa:sa + la] = False
    other[sc:sc + lc] = False
    assert np.array_equal(rt[other], base[other])
