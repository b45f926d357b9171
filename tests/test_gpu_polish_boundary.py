"""GPU: the kernels around the polishing walk -- seg_init (which also presets the arrive slots, the ticket, the candidate count and
the flags), seg_summary, seg_finish (gather + stitch over 4 KiB pieces) and find_cuts -- at the smallest shapes at which they can go
wrong.  One batch per k (boundary_batch) holds them all; every comparison is exact equality with the CPU oracle: texts, CSV rows
(the fix records with their aux bytes written out) and the QV counters, per batch and per chunk.

What the batch holds, and why:
  * chunks of 64, 65 and 129 segments (two of the last): the summary's prefix sums go 64 segments at a time;
  * chunks of k - 1, k and k + 1 bases, of 1, 15, 16 and 17 bases and of none: no window, one window, two; owned ranges on both
    sides of the stitch's 16-byte block;
  * chunks with records between chunks without: the gather adds up the records of the chunks in front of its own;
  * substitutions at a chunk's first and last base and at every offset inside a 16-byte block (the gap of the segment's buffer
    stands where the last edit was);
  * a chunk whose only segment makes 32 edits and one that makes 33 (STITCH_MAX_EDITS: traced through the edit list / flagged whole);
  * inserted and deleted bases next to multiples of 64, more than TMIN apart: every one is a segment boundary, the text behind it
    moves, and two segments share a 64-position flag tile in the new text.
Passes 1, 2 and 4 (the later passes have far fewer segments than pass 0: nothing may be left over from the pass before), fix=False,
1 and 3 lanes, the host's bookkeeping, the redo (with and without room), and a second, smaller call on the same table."""
import contextlib
import os

import pytest

import polish_plant as P

pytestmark = pytest.mark.gpu
HEADER = "Contig Base_coord Original Mutation\r\n"
KNOBS = ("JASPER_POLISH_LANES", "JASPER_POLISH_HOST_BOOKKEEPING", "JASPER_POLISH_TEST_REDO", "JASPER_POLISH_TEST_REDO_NOROOM",
         "JASPER_POLISH_TIGHT")
KS = (21, 37)
SPACING = 1030                # between the substitutions of the many-segment chunks: just above TMIN, every one a sync point


@contextlib.contextmanager
def knobs(**kw):
    assert set(kw) <= {k[len("JASPER_POLISH_"):] for k in KNOBS}
    for name in KNOBS:
        os.environ.pop(name, None)
    os.environ.update({"JASPER_POLISH_" + k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for name in KNOBS:
            os.environ.pop(name, None)


def mutate(text, edits):
    """text with errors: (pos, 's') another base at pos, (pos, 'i') a base inserted in front of pos, (pos, 'd') the base at pos lost"""
    t = list(text)
    for pos, kind in sorted(edits, reverse=True):
        other = "ACGT"[("ACGT".index(t[pos]) + 1) % 4]
        if kind == "s":
            t[pos] = other
        elif kind == "i":
            t.insert(pos, other)
        else:
            del t[pos]
    return "".join(t)


def boundary_batch(k):
    """dict(reads, names, seqs, many: {chunk index: segments in pass 0}, edits: {chunk index: substitutions in its one segment},
    small: indices of a smaller batch for a second call)"""
    T = P.geometry(k)["TMIN"]
    assert SPACING >= T
    tr = P.truth(k, 470_000, 500 + k)
    at = [P.LO]
    chunks, many, edits = [], {}, {}

    def take(length, subs_rel):
        lo = at[0]
        at[0] += length + 64
        chunks.append((lo, lo + length, [lo + e for e in subs_rel]))
        return len(chunks) - 1

    def many_segments(n):
        # the BAD run of a substitution at e starts at window e - k + 1: cuts at SPACING, 2 * SPACING, ...
        many[take(n * SPACING, [SPACING * j + k - 1 for j in range(1, n)])] = n

    many_segments(64)
    take(k - 1, [])
    many_segments(65)
    take(k, [])
    many_segments(129)
    take(k + 1, [])
    many_segments(129)
    for n in (1, 15, 16, 17, 0):
        take(n, [])
    # the first and the last base, and one substitution at every offset of a 16-byte block (too close to the ends for a cut)
    take(2 * T, [0, 2 * T - 1] + [100 + 97 * j for j in range(16)])
    for n in (32, 33):                                                  # one segment (no window count above 2 * TMIN), n edits
        c = take(n * (k + 8) + 3 * k, [2 * k + (k + 8) * j for j in range(n)])
        assert chunks[c][1] - chunks[c][0] - k + 1 <= 2 * T
        edits[c] = n
    plant = P.Plant(k, tr, (), chunks, name="b")
    names, seqs = plant.names(), plant.seqs()
    # inserted and lost bases around multiples of 64, each the start of a segment of its own
    lo = at[0]
    indels = [(1500 * (j + 1) + 64 * j + d, "id"[j % 2]) for j, d in enumerate((-1, 0, 1, -1, 0, 1, 31, 32))]
    names.append("indels:%d" % lo)
    seqs.append(mutate(tr[lo:lo + 14_000], indels))
    lo += 14_064
    names.append("clean:%d" % lo)                                       # nothing to fix
    seqs.append(tr[lo:lo + 5000])
    assert lo + 5000 <= len(tr)
    small = list(range(len(chunks) - 3, len(names)))                    # the first-and-last chunk, 32, 33, the indels, the clean one
    return dict(k=k, reads=plant.reads(), names=names, seqs=seqs, many=many, edits=edits, small=small, plant=plant)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


@pytest.fixture(scope="module")
def worlds(KT):
    """per k: the batch, its table, the oracle's map, and the oracle's answers by (chunk indices, passes, fix) -- computed once"""
    from oracle import oracle as O
    made = {}

    def get(k):
        if k not in made:
            b = boundary_batch(k)
            t = KT(k, min_slots=1 << 21)
            t.count_bases(b["reads"])
            db = O.OracleDB(k)
            db.count_bases(b["reads"])
            made[k] = dict(b, t=t, db=db, answers={})
            check_shapes(made[k])
        return made[k]
    yield get
    for w in made.values():
        w["t"].close()


def oracle_answer(w, passes, fix=True, which=None):
    key = (tuple(which) if which is not None else None, passes, fix)
    if key not in w["answers"]:
        names, seqs = pick(w, which)
        fixed, rows, qv, _ = w["db"].polish_batch(names, seqs, P.THRE, passes, fix=fix)
        w["answers"][key] = (fixed, [HEADER + r for r in rows] if fix else None, qv)
    return w["answers"][key]


def pick(w, which):
    if which is None:
        return w["names"], w["seqs"]
    return [w["names"][i] for i in which], [w["seqs"][i] for i in which]


def check_shapes(w):
    """the batch is what its description says: segment counts by the restated cut rule, edit counts by the oracle's records"""
    k, plant = w["k"], w["plant"]
    geo = P.geometry(k)
    for c, n in w["many"].items():
        lo, hi, _ = plant.chunks[c]
        assert len(P.cuts(plant.classes(c, 0), hi - lo, k, geo)) + 1 == n
    fixed, rows, _ = oracle_answer(w, 1)
    for c, n in w["edits"].items():
        assert sum(1 for line in rows[0].split("\r\n") if line.startswith(w["names"][c] + " ")) == n
        assert fixed[c] == plant.truth[plant.chunks[c][0]:plant.chunks[c][1]]
    i = w["names"].index([n for n in w["names"] if n.startswith("indels:")][0])
    lo = int(w["names"][i].split(":")[1])
    assert oracle_answer(w, 2)[0][i] == plant.truth[lo:lo + 14_000]      # two passes remove every inserted base and restore every lost one


def polish(w, passes, fix=True, which=None, **kw):
    from jasper_amd import polisher
    names, seqs = pick(w, which)
    with knobs(**kw):
        fixed, rows, qv, res = polisher.polish_batch(w["t"], names, seqs, P.THRE, passes, fix=fix)
    return fixed, [polisher.fix_csv_text(r) for r in rows], qv, res


def assert_equals_oracle(w, got, passes, fix=True, which=None):
    fixed, rows, qv, res = got
    fixed_o, rows_o, qv_o = oracle_answer(w, passes, fix, which)
    names, _ = pick(w, which)
    assert qv == qv_o
    for c, (a, b) in enumerate(zip(fixed, fixed_o)):
        assert a == b, "text of chunk %d (%s) differs" % (c, names[c])
    if fix:
        assert rows == rows_o
    else:
        assert not res.records and all(r == HEADER for r in rows)
    # (the oracle has no per-chunk output: the chunks' counters add up to the batch's)
    assert [sum(res.qv_chunk(c)[q] for c in range(len(names))) for q in range(4)] == list(qv_o)


def everything(res, n):
    return (res.seqs, res.records, res.qv, [res.qv_chunk(i) for i in range(n)], res.segments, res.lookups)


@pytest.mark.parametrize("passes", [1, 2, 4])
@pytest.mark.parametrize("k", KS)
def test_batch_equals_oracle(worlds, k, passes):
    w = worlds(k)
    got = polish(w, passes, LANES=1)
    assert_equals_oracle(w, got, passes)
    assert any(r["kind"] != "s" for r in got[3].records)                # (the indels were repaired as indels)


@pytest.mark.parametrize("k", KS)
def test_no_fix(worlds, k):
    w = worlds(k)
    assert_equals_oracle(w, polish(w, 2, fix=False, LANES=1), 2, fix=False)


@pytest.mark.parametrize("k", KS)
def test_three_lanes(worlds, k):
    w = worlds(k)
    n = len(w["seqs"])
    one, three = polish(w, 2, LANES=1), polish(w, 2, LANES=3)
    assert_equals_oracle(w, three, 2)
    assert everything(three[3], n) == everything(one[3], n)


@pytest.mark.parametrize("knob", [dict(HOST_BOOKKEEPING=1), dict(TEST_REDO="all"), dict(TEST_REDO="all", TEST_REDO_NOROOM=1),
                                  dict(HOST_BOOKKEEPING=1, LANES=3)], ids=["host_bookkeeping", "redo", "redo_noroom", "host_bookkeeping_3_lanes"])
@pytest.mark.parametrize("k", KS)
def test_rare_paths(worlds, k, knob):
    w = worlds(k)
    n = len(w["seqs"])
    got = polish(w, 2, **dict(dict(LANES=1), **knob))
    assert_equals_oracle(w, got, 2)
    want = polish(w, 2, LANES=1)[3]
    assert (got[3].seqs, got[3].records, got[3].qv, [got[3].qv_chunk(i) for i in range(n)]) == \
           (want.seqs, want.records, want.qv, [want.qv_chunk(i) for i in range(n)])


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("k", KS)
def test_smaller_call_after_larger(worlds, k, lanes):
    """the second call has fewer segments and fewer candidates than the first: arrive slots, ticket, count and flags of the first
    must not show"""
    w = worlds(k)
    big = polish(w, 2, LANES=lanes)
    small = polish(w, 2, which=w["small"], LANES=lanes)
    assert small[3].segments < big[3].segments
    assert_equals_oracle(w, small, 2, which=w["small"])
    assert_equals_oracle(w, polish(w, 1, which=w["small"][-1:], LANES=1), 1, which=w["small"][-1:])      # ... and one clean chunk alone
