"""GPU: the list passes of the counting path (count_part.hip) on text WITHOUT read boundaries, against an exact count of the stream.

Reads of 150 bases give a 16384-base tile about 12.4 K records, which part1_kernel stages in one round; an assembly gives it 16384,
and the front end then stages in rounds, copies out with a running first record, and -- once a slice is full -- does so record by
record.  Here every text is megabases without an invalid byte (or with single invalid bytes planted at chosen distances from the
tile seams), counted through the partitioned path into a table of 2^24 slots, the smallest that takes it, and compared entry for
entry with stream_ref.count_stream: numpy on the text alone, no kernel, no shared encoding, canonical choice or hash code.

Texts (stream_ref.py): a random genome of 2 000 003 bases repeated end to end (2 M keys of count 4 and 5, each at four or five
different tile offsets); the same with an invalid byte before and after every tile boundary and 3 % lower case; the same with a
run of `A` and one of `AC` longer than a tile, which fill a slice of the first list level; the seam text extended to two pieces.
"""
import contextlib
import os
import re

import numpy as np
import pytest

import layout_util as lu
import stream_ref as sr

pytestmark = pytest.mark.gpu

S = 24                                   # log2 slots: pieces below 8 MiB take the direct kernel, and 8 Mi bases need this table
TILE = 16384                             # count_part.hip: PT_TILE
P1_STAGE, P1W_STAGE = 13824, 6912        # records per staging round of part1_kernel / of a half tile in part1w_kernel
PERIOD = 2_000_003
LEN = 8 * 2**20 + 3 * TILE + 5
ROOM = 3 * (1 << S) // 4                 # the first piece of a call into an empty table: 12 582 912 bases
LEN_LONG = ROOM + 8 * 2**20 + 2 * TILE + 7
KS = [16, 32, 33, 37, 38, 48, 49, 64]    # part1<1>, <2>, <3>, <3, 37>, part1w<3> (narrow table), part1w<3> (wide), part1w<4>, 2k = 128
KS2 = [37, 49]
RUN_TILES = (76, 175)                    # where the two runs of the full-slice text start (100 bases before these tile boundaries)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


@pytest.fixture(scope="module")
def cache():
    """texts, their references and their device copies, made once per module"""
    c = {}
    yield c
    c.clear()


def cached(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


def text_of(cache, name, k=None):
    """-> (text, what the builder planted)"""
    if name == "base":
        return cached(cache, ("text", name), lambda: (sr.base_text(ROOM, PERIOD), None))          # (the longest N-free text any case counts)
    if name == "seam":
        return cached(cache, ("text", name, k), lambda: sr.seam_text(text_of(cache, "base")[0][:LEN], k, TILE))
    if name == "runs":
        return cached(cache, ("text", name), lambda: sr.run_text(text_of(cache, "base")[0][:LEN], TILE, *RUN_TILES))
    assert name == "long"
    return cached(cache, ("text", name, k), lambda: sr.seam_text(sr.base_text(LEN_LONG, PERIOD), k, TILE))


def ref_of(cache, name, k, n=LEN):
    """count_stream of the first n bytes of a text (the long text: all of it); a text that extends another pays for the rest only"""
    def make():
        if name == "long":
            text, short = text_of(cache, "long", k)[0], text_of(cache, "seam", k)[0]
            assert np.array_equal(text[:LEN], short)
            return sr.add(ref_of(cache, "seam", k), sr.count_stream(text[LEN - k + 1:], k))
        text = text_of(cache, name, k)[0]
        if n > LEN:
            return sr.add(ref_of(cache, name, k), sr.count_stream(text[LEN - k + 1:n], k))
        return sr.count_stream(text[:n], k)
    return cached(cache, ("ref", name, k, n), make)


def dev_of(cache, name, k=None):
    import torch

    def make():
        d = torch.from_numpy(np.ascontiguousarray(text_of(cache, name, k)[0])).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        return d
    return cached(cache, ("dev", name, None if name in ("base", "runs") else k), make)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def new_table(KT, k):
    t = KT(k, min_slots=1 << S)
    assert t.info()["slots"] == 1 << S
    return t


PIECE = re.compile(r"\[count\] partitioned piece (\d+) bases: p1 (\d+) p2 (\d+) rbits (\d+) nblk1 (\d+) nblk2 (\d+) cap1 (\d+) cap2 (\d+) "
                   r"\| fullest slice1 (\d+) slice2 (\d+) deferred (\d+)")
FIELDS = ("len", "p1", "p2", "rbits", "nblk1", "nblk2", "cap1", "cap2", "slice1", "slice2", "deferred")


def count(t, ptr, n, capfd):
    """one counting call -> the geometry of each partitioned piece, as the debug line prints it, with part1's grid worked out
    as Table::partition_geometry does"""
    capfd.readouterr()
    with env(JASPER_COUNT_DEBUG="2"):
        t.count_bases_device(ptr, n)
    log = capfd.readouterr().err
    assert "piece abandoned" not in log, log[-600:]
    assert t.info()["slots"] == 1 << S
    geoms = []
    for m in PIECE.finditer(log):
        g = dict(zip(FIELDS, map(int, m.groups())))
        g["ntiles"] = (g["len"] + TILE - 1) // TILE
        g["grid1"] = max(1, min(g["len"] // ((1 << g["p1"]) * 512), g["ntiles"], 256))
        g["per_block"] = (g["ntiles"] + g["grid1"] - 1) // g["grid1"]
        geoms.append(g)
    return geoms


def explain(text, k, got, want, geoms):
    """the first differing keys, decoded, and where their windows END in the text: tile, offset in the tile, first tile of a block or
    not (tiles and blocks of a call's first piece; a later piece starts k-1 bases, rounded down to 16 bytes, before its first base)"""
    g = {(int(a), int(b)): int(c) for a, b, c in zip(*got)}
    w = {(int(a), int(b)): int(c) for a, b, c in zip(*want)}
    bad = sorted(key for key in set(g) | set(w) if g.get(key) != w.get(key))
    hi, lo, valid = sr.window_hashes(text, k)
    per_block = geoms[0]["per_block"] if geoms else 0
    lines = ["%d keys differ; pieces of the last call: %s" % (len(bad), [(x["len"], x["grid1"], x["per_block"]) for x in geoms])]
    for key in bad[:5]:
        ends = np.flatnonzero(valid & (hi == np.uint64(key[0])) & (lo == np.uint64(key[1]))) + (k - 1)
        where = ["pos %d = tile %d + %d%s" % (e, e // TILE, e % TILE, " (block-first)" if per_block and (e // TILE) % per_block == 0 else "")
                 for e in ends.tolist()[:8]]
        lines.append("%s: table %s, reference %s; windows end at %s" % (lu.decode(k, (key[0] << 64) | key[1]), g.get(key), w.get(key), where))
    return "\n".join(lines)


def right_filled(window, k):
    """what lookup() makes of a string: cut at the first byte that is no base, filled up with A"""
    s = ""
    for v in window:
        if sr._CODE[v] == 255:
            break
        s += chr(v).upper()
    return s + "A" * (k - len(s))


def seam_windows(text, k, plants):
    """window starts around the tile boundaries: ~1000 that are k-mers, and those that hold a planted byte"""
    n = text.size
    valid = sr.valid_windows(text, k)
    starts = set()
    for T in range(1, (n + TILE - 1) // TILE):
        for d in ((T * 7) % (k + 66), (T * 13 + 5) % (k + 66), (T * 29 + 11) % (k + 66), -((T * 5) % 48), k - 1, 0):
            s = T * TILE - d
            if 0 <= s <= n - k:
                starts.add(s)
    clean = sorted(s for s in starts if valid[s])
    clean = clean[::max(1, len(clean) // 1000)]
    holed = sorted(s for s in starts if not valid[s])
    for p, _, _, _ in (plants or [])[:120]:
        holed += [s for s in (p, p - 1, p - k // 2, p - k + 1) if 0 <= s <= n - k]
    return clean, sorted(set(holed))


def check(t, text, ref, k, geoms, pieces, plants=None, first_call=False):
    """every comparison of the table with the reference of all that was counted into it; `text` is the text of the last call,
    `pieces` the number of its pieces"""
    wide = lu.is_wide(k, S)
    assert t.count_path() == 1 and t.count_stages()[1] == pieces, "the list passes were not taken for every piece"
    want_histo = sr.histogram(ref)
    if first_call:
        assert t.histogram_is_fused() == (not wide)
        assert t.histogram() == want_histo, "the histogram binned while the counts were written"
        t.import_entries(np.array([[ref[0][0], ref[1][0], 0]], dtype=np.uint64))          # (adds nothing, drops the fused histogram)
        assert not t.histogram_is_fused()
    e = t.export_entries()
    order = np.lexsort((e[:, 1], e[:, 0]))
    got = tuple(np.ascontiguousarray(e[order, i]) for i in range(3))
    if not sr.same(got, ref):
        pytest.fail("export_entries differs from the stream's count, k = %d:\n%s" % (k, explain(text, k, got, ref, geoms)), pytrace=False)
    info = t.info()
    assert info["distinct"] == ref[0].size
    assert info["occurrences"] == int(ref[2].sum())
    assert t.histogram() == want_histo
    clean, holed = seam_windows(text, k, plants)
    assert len(clean) >= 900
    strings = [bytes(text[s:s + k]) for s in clean]
    want = [min(sr.lookup(ref, lu.hash_of_kmer(w.decode().upper())), lu.U32) for w in strings]
    assert min(want) >= 1
    assert t.lookup(strings) == want
    assert t.lookup([lu.revcomp(w.decode().upper()) for w in strings]) == want
    if plants:
        assert len(holed) >= 300
        strings = [bytes(text[s:s + k]) for s in holed]
        assert t.lookup(strings) == [min(sr.lookup(ref, lu.hash_of_kmer(right_filled(w, k))), lu.U32) for w in strings]


def assert_rounds(text, k, every_tile=False):
    """the staging takes several rounds: derived from the valid windows per tile, not assumed"""
    both, h0, h1 = sr.tile_records(text, k, TILE)
    assert both.max() > P1_STAGE, "no tile with more records than one staging round of part1_kernel holds"
    if k >= 38:
        assert max(h0.max(), h1.max()) > P1W_STAGE, "no half tile with more records than one staging round of part1w_kernel holds"
    if every_tile:                                                                   # (but the last tile, which is a few bases)
        assert both[:-1].min() > P1_STAGE and (k < 38 or np.minimum(h0, h1)[:-1].min() > P1W_STAGE)


# ---- 1. text without an invalid byte ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_text_without_read_boundaries(KT, cache, capfd, k):
    """8 Mi + 3 tiles + 5 bases without an invalid byte: every tile is staged in rounds (two per tile; two per half for k >= 38),
    the last tile is partial.  Into an empty table, then once more into the filled one (images loaded from HBM).  k = 37, 49: also
    a length that is a multiple of the tile, and one that is a multiple of 16 only."""
    text = text_of(cache, "base")[0]
    ref = ref_of(cache, "base", k)
    assert_rounds(text[:LEN], k, every_tile=True)
    assert int(ref[2].sum()) == LEN - k + 1 and set(np.unique(ref[2]).tolist()) >= {4, 5}
    d = dev_of(cache, "base")
    t = new_table(KT, k)
    geoms = count(t, d.data_ptr(), LEN, capfd)
    assert len(geoms) == 1 and geoms[0]["len"] == LEN
    check(t, text[:LEN], ref, k, geoms, 1, first_call=True)
    geoms = count(t, d.data_ptr(), LEN, capfd)
    assert len(geoms) == 1
    check(t, text[:LEN], sr.times(ref, 2), k, geoms, 1)
    t.close()
    if k in KS2:
        for n in (8 * 2**20 + 4 * TILE, 8 * 2**20 + 3 * TILE + 16 * 7):
            assert n % 16 == 0 and LEN < n <= ROOM
            t = new_table(KT, k)
            geoms = count(t, d.data_ptr(), n, capfd)
            assert len(geoms) == 1 and geoms[0]["len"] == n
            check(t, text[:n], ref_of(cache, "base", k, n), k, geoms, 1, first_call=True)
            t.close()


# ---- 2. invalid bytes at chosen distances from the tile seams --------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_invalid_bytes_around_tile_seams(KT, cache, capfd, k):
    """one invalid byte before and one after EVERY tile boundary, at the distances where a thread's validity mask changes hands:
    its own 16 bases, the 64 before them, k and k +- 1; every byte value that is no base; 3 % lower case.  A block's first tile
    reads the 64 bases before it from memory, its later tiles from words parked in LDS: each distance is checked to occur at both."""
    text, plants = text_of(cache, "seam", k)
    ref = ref_of(cache, "seam", k)
    assert_rounds(text, k, every_tile=True)
    values = [v for _, v, _, _ in plants]
    assert set(values) == set(sr.INVALID_BYTES) and min(values.count(v) for v in sr.INVALID_BYTES) >= 2
    assert int(ref[2].sum()) == int(sr.valid_windows(text, k).sum()) < LEN - k + 1 - len(plants)
    d = dev_of(cache, "seam", k)
    t = new_table(KT, k)
    geoms = count(t, d.data_ptr(), LEN, capfd)
    assert len(geoms) == 1 and geoms[0]["len"] == LEN
    per_block = geoms[0]["per_block"]
    assert per_block == (33 if k >= 37 else 3), geoms
    for offs in (sr.before_offsets(k), sr.after_offsets(k)):
        for off in set(offs):
            at = [T for _, _, T, o in plants if o == off and o in offs]
            assert sum(T % per_block == 0 for T in at) >= 1, "offset %d occurs at no block's first tile" % off
            assert sum(T % per_block != 0 for T in at) >= 3, "offset %d occurs at fewer than three ordinary boundaries" % off
    check(t, text, ref, k, geoms, 1, plants=plants, first_call=True)
    t.close()


# ---- 3. a full slice and several rounds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS2)
def test_full_slice_with_several_rounds(KT, cache, capfd, k):
    """a run of 16384 + 200 `A` and one of `AC`, each across three tiles of one block: one or two keys whose records exceed a slice of
    their bucket's list.  From then on the block copies out record by record, against the slice's bound and with the running first
    record of a staging round, and what does not fit goes to the deferred list."""
    text, runs = text_of(cache, "runs")
    ref = ref_of(cache, "runs", k)
    assert_rounds(text, k)
    run_len = runs[0][1]
    assert run_len == TILE + 200 and int(ref[2].max()) >= run_len - k + 1
    d = dev_of(cache, "runs")
    t = new_table(KT, k)
    geoms = count(t, d.data_ptr(), LEN, capfd)
    assert len(geoms) == 1
    g = geoms[0]
    blocks = [{(s // TILE) // g["per_block"], ((s + n - 1) // TILE) // g["per_block"]} for s, n in runs]
    assert all(len(b) == 1 for b in blocks) and blocks[0] != blocks[1], "each run within one block's tiles, the two in different blocks"
    assert g["cap1"] < run_len
    assert g["deferred"] >= 2 * (TILE - g["cap1"])
    assert g["deferred"] <= max(65536, LEN // 48) // 2
    check(t, text, ref, k, geoms, 1, first_call=True)
    t.close()


# ---- 4. two pieces, and a text that is not 16-byte aligned ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS2)
def test_second_piece_and_misaligned_text(KT, cache, capfd, k):
    """one call of 12 582 912 + 8 Mi + 2 tiles + 7 bases: the first piece takes the table's whole room, the second starts k-1 bases
    early, rounded down to a 16-byte address, and goes through the list passes into the filled table.  From a buffer shifted by
    0, 1 and 9 bytes: the second piece's first counted window moves, and part1's 16-byte text loads are unaligned."""
    import torch
    text, plants = text_of(cache, "long", k)
    ref = ref_of(cache, "long", k)
    assert text.size == LEN_LONG and LEN_LONG - ROOM >= 8 << 20
    src = torch.from_numpy(np.ascontiguousarray(text)).to(torch.device("cuda", 0))
    buf = torch.full((LEN_LONG + 32,), ord("A"), dtype=torch.uint8, device=src.device)
    assert buf.data_ptr() % 16 == 0
    starts = set()
    for shift in (0, 1, 9):
        buf.fill_(ord("A"))
        view = buf[shift:shift + LEN_LONG]
        view.copy_(src)
        torch.cuda.synchronize()
        t = new_table(KT, k)
        geoms = count(t, view.data_ptr(), LEN_LONG, capfd)
        assert [g["len"] for g in geoms][:1] == [ROOM] and len(geoms) == 2, geoms
        start = LEN_LONG - geoms[1]["len"]                                   # where the second piece's text begins
        assert ROOM - (k - 1) - 15 <= start <= ROOM - (k - 1) and (start + shift) % 16 == 0
        starts.add(ROOM - start)
        check(t, text, ref, k, geoms, 2, plants=plants)
        t.close()
    assert len(starts) == 3, "three different first counted windows (emit_from) of the second piece"
    del buf, src
