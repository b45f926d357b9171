"""An exact count of every canonical k-mer of a whole base stream, in hash space, and the planted texts of tests/test_gpu_count_text.py.

count_stream(text, k) is numpy on whole arrays and owes nothing to the library: a byte is a base iff it is one of ACGTacgt, a window
counts iff all of its k bytes are bases, the first base is the most significant bit pair, canonical is the numeric minimum of the
two strands, and the hash is the one layout_util.py_mix restates.  The two 64-bit key words of every window are built by doubling
(1 -> 2 -> 4 ... -> 32 bases packed into a word), the reverse strand from the reversed complement TEXT, all in unsigned 64-bit
integers (a multiplication wraps modulo 2^64, which is what the hash asks for).  About 5 s for 8 M windows.

A reference is the triple (hi, lo, count) of uint64 arrays sorted by (hi, lo): the mixed hash of each distinct canonical k-mer and
its occurrences.  Counts are additive over a cut with k-1 bases of overlap:  count_stream(t) = add(count_stream(t[:a]),
count_stream(t[a-k+1:])), so a text that extends another pays for the extension only.
"""
import numpy as np

import layout_util as lu

HISTO_BINS = lu.HISTO_BINS
_C1 = np.uint64(lu._C1)
_ONES = np.uint64(lu.M64)

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _i
    _CODE[ord(_ch.lower())] = _i
INVALID_BYTES = [v for v in range(256) if _CODE[v] == 255]          # the 248 byte values that are no base
assert len(INVALID_BYTES) == 248


def as_array(text):
    if isinstance(text, np.ndarray):
        return text.astype(np.uint8, copy=False)
    if isinstance(text, str):
        text = text.encode("latin-1")
    return np.frombuffer(bytes(text), dtype=np.uint8)


def _u(x):
    return np.uint64(x)


def _packed(c, m):
    """the m <= 32 bases c[i:i+m] as one word, first base on top, for every i: powers of two by doubling, then m's binary digits"""
    assert 1 <= m <= 32 and c.size >= m
    n = c.size - m + 1
    pw, s = {1: c}, 1
    while 2 * s <= m:
        p = pw[s]
        pw[2 * s] = (p[:-s] << _u(2 * s)) | p[s:]
        s *= 2
    out, off = None, 0
    while s:
        if m & s:
            part = pw[s][off:off + n]
            out = part.copy() if out is None else (out << _u(2 * s)) | part
            off += s
        s >>= 1
    return out


def _key_words(c, k):
    """(hi, lo) of the 2k-bit key of every window c[i:i+k]; hi is None for k <= 32"""
    n = c.size - k + 1
    if k <= 32:
        return None, _packed(c, k)
    return _packed(c, k - 32)[:n], _packed(c, 32)[k - 32:k - 32 + n]


def _mix(hi, lo, k):
    """layout_util.py_mix on arrays"""
    B = 2 * k
    if B <= 64:
        m = _ONES if B == 64 else _u((1 << B) - 1)
        v = lo & m
        v ^= v >> _u(k)
        v = (v * _C1) & m
        v ^= v >> _u(k)
        return np.zeros_like(v), v
    hb = B - 64
    lo = lo ^ (lo >> _u(32))
    lo = lo * _C1
    lo ^= lo >> _u(29)
    rot = (lo >> _u(30)) | (lo << _u(34))
    return (hi ^ rot) & (_ONES if hb == 64 else _u((1 << hb) - 1)), lo


def valid_windows(text, k):
    """bool per window start i: all of text[i:i+k] are bases"""
    b = as_array(text)
    if b.size < k:
        return np.zeros(0, dtype=bool)
    bad = np.concatenate([[0], np.cumsum(_CODE[b] == 255, dtype=np.int64)])
    return bad[k:] == bad[:-k]


def window_hashes(text, k):
    """(hi, lo, valid) per window start: the mixed hash of the canonical k-mer (meaningless where valid is False)"""
    assert 1 <= k <= 64
    b = as_array(text)
    valid = valid_windows(b, k)
    if valid.size == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, z.copy(), valid
    code = _CODE[b]
    c = np.where(code == 255, 0, code).astype(np.uint64)
    fhi, flo = _key_words(c, k)
    rc = np.ascontiguousarray((_u(3) - c)[::-1])          # the reversed complement text: its window n-1-i is window i's other strand
    rhi, rlo = _key_words(rc, k)
    rlo = rlo[::-1]
    if fhi is None:
        lo = np.minimum(flo, rlo)
        hi = None
    else:
        rhi = rhi[::-1]
        take_r = (rhi < fhi) | ((rhi == fhi) & (rlo < flo))
        hi = np.where(take_r, rhi, fhi)
        lo = np.where(take_r, rlo, flo)
    hi, lo = _mix(hi, lo, k)
    return hi, lo, valid


def _reduce(hi, lo, cnt):
    """sort by (hi, lo) and add up the counts of equal keys"""
    if lo.size == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, z.copy(), z.copy()
    order = np.lexsort((lo, hi)) if hi.any() else np.argsort(lo, kind="stable")
    hi, lo, cnt = hi[order], lo[order], cnt[order]
    first = np.flatnonzero(np.concatenate([[True], (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])]))
    return hi[first], lo[first], np.add.reduceat(cnt, first).astype(np.uint64)


def count_stream(text, k):
    """(hi, lo, count): sorted uint64 arrays, the mixed hash of every canonical k-mer of the stream and its occurrences"""
    hi, lo, valid = window_hashes(text, k)
    hi, lo = hi[valid], lo[valid]
    return _reduce(hi, lo, np.ones(lo.size, dtype=np.uint64))


def add(a, b):
    return _reduce(*(np.concatenate([x, y]) for x, y in zip(a, b)))


def times(a, m):
    return a[0], a[1], a[2] * _u(m)


def histogram(ref):
    return np.bincount(np.minimum(ref[2], _u(HISTO_BINS - 1)).astype(np.int64), minlength=HISTO_BINS).tolist()


def lookup(ref, h):
    """count of the key with mixed hash h (a Python int), 0 if absent"""
    hi, lo, cnt = ref
    a, b = np.searchsorted(hi, _u(h >> 64), "left"), np.searchsorted(hi, _u(h >> 64), "right")
    i = a + np.searchsorted(lo[a:b], _u(h & lu.M64), "left")
    return int(cnt[i]) if i < b and int(lo[i]) == h & lu.M64 else 0


def from_counter(counter, k):
    """a layout_util.kmer_counter (canonical k-mer string -> count) as a reference: strings through int_of_kmer and py_mix"""
    hs = [(lu.py_mix(lu.int_of_kmer(km), 2 * k), c) for km, c in counter.items()]
    hs.sort()
    return (np.array([h >> 64 for h, _ in hs], dtype=np.uint64), np.array([h & lu.M64 for h, _ in hs], dtype=np.uint64),
            np.array([c for _, c in hs], dtype=np.uint64))


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def tile_records(text, k, tile):
    """records per tile as the front end sees them: a window belongs to the tile (and, of its thread's 16 bases, to the half of 8)
    of its LAST base.  -> (per tile, per tile in first halves, per tile in second halves)"""
    v = valid_windows(text, k)
    n = as_array(text).size
    nt = (n + tile - 1) // tile
    end = np.flatnonzero(v) + (k - 1)
    first_half = (end & 15) < 8
    both = np.bincount(end // tile, minlength=nt)
    h0 = np.bincount(end[first_half] // tile, minlength=nt)
    return both, h0, both - h0


# ---- the texts ----------------------------------------------------------------------------------------------------------------------
def base_text(length, period, seed=20240):
    """a random genome of `period` bases over ACGT, repeated end to end without a separator and cut to `length`"""
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, period)]
    return np.resize(g, length)


def before_offsets(k):
    return [-65, -64, -63, -k - 1, -k, -k + 1, -17, -16, -15, -1]


def after_offsets(k):
    return [0, 1, 15, 16, 17, k - 2, k - 1]


def seam_text(base, k, tile):
    """`base` with, at every tile boundary T * tile inside it, one invalid byte before the boundary (the offsets of before_offsets,
    cycling with T) and one after it (after_offsets, cycling on their own); the planted values cycle through INVALID_BYTES; 3 % of
    the other bases in lower case, chosen by position (so that a longer text's prefix is the shorter text).
    -> (text, plants): plants = [(position, byte value, T, offset)], each position once (a later plant on the same position wins)"""
    t = base.copy()
    pos = np.arange(t.size, dtype=np.uint64)
    lower = ((pos * _u(2654435761) + _u(12345)) >> _u(8)) % _u(100) < _u(3)
    t[lower] |= 0x20
    bo, ao = before_offsets(k), after_offsets(k)
    at, nv = {}, 0
    for T in range(1, (t.size + tile - 1) // tile):
        for off in (bo[(T - 1) % len(bo)], ao[(T - 1) % len(ao)]):
            p = T * tile + off
            if 0 <= p < t.size:
                at[p] = (INVALID_BYTES[nv % len(INVALID_BYTES)], T, off)
                nv += 1
    for p, (v, _, _) in at.items():
        t[p] = v
    return t, sorted((p, v, T, off) for p, (v, T, off) in at.items())


def run_text(base, tile, tile_a, tile_ac, extra=200, lead=100):
    """`base` with a run of tile + extra times `A` that starts `lead` bases before the boundary tile_a * tile, and an equally long run
    of `AC` repeated placed the same way at tile_ac * tile.  -> (text, [(start, length) of the two runs])"""
    t = base.copy()
    n = tile + extra
    runs = []
    for T, unit in ((tile_a, b"A"), (tile_ac, b"AC")):
        s = T * tile - lead
        assert 0 <= s and s + n <= t.size
        t[s:s + n] = np.resize(np.frombuffer(unit, dtype=np.uint8), n)
        runs.append((s, n))
    return t, runs
