"""CPU: the restated cut rule of tests/polish_plant.py on hand-worked class arrays, and -- with the oracle alone -- what
tests/test_gpu_polish_paths.py takes for granted about its plants: a fixing pass restores the truth (so the class map of the
later passes is known), the walk stands on the dips it is meant to stand on, and every phase probe tells the true arrival phase
from every other one."""
import numpy as np
import pytest

import polish_plant as P

GEO = {"TMIN": 1024, "CMIN": 32768, "CLEAN_CELL": 65536, "W": 16, "M": 12}       # hand-worked arrays: k = 4


def _cls(n, bad=()):
    c = np.zeros(n, dtype=np.uint8)
    for a, b in bad:
        c[a:b] = P.BAD
    return c


def test_geometry_query():
    from jasper_amd import _lib
    import ctypes as C
    for k in (1, 21, 37, 64):
        g = P.geometry(k)
        assert g["W"] == 4 * k and g["M"] == 3 * k and g["TMIN"] > 5 * 64 and g["CMIN"] >= g["TMIN"]
        assert g["CLEAN_CELL"] >= 2 * g["CMIN"] and g["CLEAN_CELL"] % 64 == 0
    out = (C.c_int64 * 5)()
    assert _lib.lib().jasper_polish_cut_geometry(0, out) != 0 and _lib.lib().jasper_polish_cut_geometry(65, out) != 0


def test_sync_candidates_by_hand():
    k, W = 4, 16
    # a run of k BAD windows from 100: the candidate is its first window
    assert P.sync_candidates(_cls(300, [(100, 104)]), k, W) == [100]
    # k-1 BAD in a row are enough, k-2 are not
    assert P.sync_candidates(_cls(300, [(100, 103)]), k, W) == [100]
    assert P.sync_candidates(_cls(300, [(100, 102)]), k, W) == []
    # W CLEAN windows before it: a BAD window at p-W-1 is allowed, at p-W not; the earlier one is a candidate itself when it is long enough
    assert P.sync_candidates(_cls(300, [(83, 84), (100, 104)]), k, W) == [100]
    assert P.sync_candidates(_cls(300, [(84, 85), (100, 104)]), k, W) == []
    assert P.sync_candidates(_cls(300, [(80, 84), (100, 104)]), k, W) == [80, 100]
    # p >= W, and p + k - 1 <= nwin
    assert P.sync_candidates(_cls(300, [(15, 19)]), k, W) == [] and P.sync_candidates(_cls(300, [(16, 20)]), k, W) == [16]
    assert P.sync_candidates(_cls(300, [(297, 300)]), k, W) == [297] and P.sync_candidates(_cls(300, [(298, 300)]), k, W) == []
    # a run that starts at window 0 has no CLEAN window before it
    assert P.sync_candidates(_cls(300, [(0, 40)]), k, W) == []


def test_clean_cells_by_hand():
    k, cell = 4, 1024
    assert P.clean_cells(_cls(1024 + 600), k, cell) == [512, 1536]
    # the text must hold [p-4k, p+k): nwin = 1536 + k is the least for the second cell
    assert P.clean_cells(_cls(1539), k, cell) == [512, -1] and P.clean_cells(_cls(1540), k, cell) == [512, 1536]
    assert P.clean_cells(_cls(515), k, cell) == [-1] and P.clean_cells(_cls(516), k, cell) == [512]
    # the outermost windows in the way: p-4k (-> p+1) and p+k-1 (-> p+5k); p-4k-1 and p+k are not in the way
    assert P.clean_cells(_cls(1000, [(496, 497)]), k, cell) == [513]
    assert P.clean_cells(_cls(1000, [(515, 516)]), k, cell) == [532]
    assert P.clean_cells(_cls(1000, [(495, 496), (516, 517)]), k, cell) == [512]
    # the LAST window in the way counts
    assert P.clean_cells(_cls(1000, [(496, 497), (500, 501)]), k, cell) == [517]
    # eight attempts, then none; seven failures leave the eighth
    assert P.clean_cells(_cls(1000, [(515 + 20 * j, 516 + 20 * j) for j in range(8)]), k, cell) == [-1]
    assert P.clean_cells(_cls(1000, [(515 + 20 * j, 516 + 20 * j) for j in range(7)]), k, cell) == [512 + 140]
    # an attempt never leaves its cell: p + k <= cell end
    assert P.clean_cells(_cls(200, [(35, 36), (43, 44)]), k, 64)[0] == 60 and P.clean_cells(_cls(200, [(35, 36), (44, 45)]), k, 64)[0] == -1


def test_cuts_by_hand():
    k, T, CM = 4, GEO["TMIN"], GEO["CMIN"]

    def run(p):
        return (p, p + k)
    L = 6000
    n = L - k + 1
    assert P.cuts(_cls(n), L, k, GEO) == []
    # TMIN between sync points: the second of two closer ones is dropped, and the next is measured from the last one KEPT
    assert P.cuts(_cls(n, [run(2000), run(2000 + T)]), L, k, GEO) == [(2000, 0), (2000 + T, 0)]
    assert P.cuts(_cls(n, [run(2000), run(1999 + T)]), L, k, GEO) == [(2000, 0)]
    assert P.cuts(_cls(n, [run(2000), run(1999 + T), run(2020 + T)]), L, k, GEO) == [(2000, 0), (2020 + T, 0)]
    # ... from the chunk start, and -- in BASES -- to the chunk end
    assert P.cuts(_cls(n, [run(T - 1)]), L, k, GEO) == [] and P.cuts(_cls(n, [run(T)]), L, k, GEO) == [(T, 0)]
    assert P.cuts(_cls(n, [run(L - T)]), L, k, GEO) == [(L - T, 0)] and P.cuts(_cls(n, [run(L - T + 1)]), L, k, GEO) == []
    # want_sync: more than 2 * TMIN windows
    L = 2 * T + k - 1
    assert P.cuts(_cls(2 * T, [run(T)]), L, k, GEO) == [] and P.cuts(_cls(2 * T + 1, [run(T)]), L + 1, k, GEO) == [(T, 0)]
    # clean cuts: more than 2 * CMIN windows, CMIN to both neighbours
    L = 2 * CM + k - 1
    assert P.cuts(_cls(2 * CM), L, k, GEO) == [] and P.cuts(_cls(2 * CM + 1), L + 1, k, GEO) == [(CM, 1)]
    L = 300_000
    n = L - k + 1
    assert P.cuts(_cls(n), L, k, GEO) == [(32768, 1), (98304, 1), (163840, 1), (229376, 1)]
    # a sync point nearer than CMIN on either side forbids the clean cut; at CMIN it does not; order is by position
    assert P.cuts(_cls(n, [run(98304 - CM + 1)]), L, k, GEO) == [(32768, 1), (98304 - CM + 1, 0), (163840, 1), (229376, 1)]
    assert P.cuts(_cls(n, [run(98304 + CM - 1)]), L, k, GEO) == [(32768, 1), (98304 + CM - 1, 0), (163840, 1), (229376, 1)]
    assert P.cuts(_cls(n, [run(98304 + CM)]), L, k, GEO) == [(32768, 1), (98304, 1), (98304 + CM, 0), (163840, 1), (229376, 1)]
    assert P.cuts(_cls(n, [run(98304 + CM + 1)]), L, k, GEO) == [(32768, 1), (98304, 1), (98304 + CM + 1, 0), (229376, 1)]
    # the last cell's cut needs CMIN bases to the chunk end
    assert P.cuts(_cls(229376 + CM - k), 229376 + CM - 1, k, GEO)[-1] == (163840, 1)
    assert P.cuts(_cls(229376 + CM - k + 1), 229376 + CM, k, GEO)[-1] == (229376, 1)
    # short and empty chunks
    assert P.cuts(_cls(0), 0, k, GEO) == [] and P.cuts(_cls(0), k - 1, k, GEO) == [] and P.cuts(_cls(4), k + 3, k, GEO) == []


def test_walk_hits_by_hand():
    k = 5                                                       # stride 4
    assert P.walk_hits(_cls(100), k) == []
    assert P.walk_hits(_cls(100, [(40, 41)]), k) == [40] and P.walk_hits(_cls(100, [(41, 42)]), k) == []
    assert P.walk_hits(_cls(100, [(40, 41), (45, 46), (51, 52)]), k) == [40, 45]        # 40 -> 41, 45 -> 46 -> 50 -> 54: 51 is passed over
    assert P.walk_hits(_cls(100, [(38, 42)]), k) == [40] and P.walk_hits(_cls(100, [(38, 42), (46, 47)]), k) == [40, 46]
    assert P.walk_hits(_cls(100, [(0, 3), (7, 8)]), k) == [0, 7]
    d = P.steer(37, 128, 128 + 2000, 128 + 32515)
    assert len(d) == 32515 % 36 and P.walk_hits(_cls(40000, [(a - 128, a - 128 + 1) for a, _ in d] + [(32515, 32516)]), 37)[-1] == 32515


# ---- the plants ------------------------------------------------------------------------------------------------------------

_DBS = {}


def _db(plant):
    """the oracle's map of a plant's reads (plants without dips share one per truth)"""
    from oracle import oracle as O
    key = (plant.k, id(plant.truth), tuple(plant.pieces))
    if key not in _DBS:
        _DBS.clear()                                            # (one at a time: the long chain's map is large)
        db = O.OracleDB(plant.k)
        db.count_bases(plant.reads())
        _DBS[key] = db
    return _DBS[key]


@pytest.mark.parametrize("k", P.KS)
def test_cut_plants_meet_their_preconditions(k):
    g = P.geometry(k)
    T, CM, CELL = g["TMIN"], g["CMIN"], g["CLEAN_CELL"]
    plants = P.cut_plants(k)
    assert sorted(plants) == sorted(P.CUT_NAMES) and sorted(P.phase_plants(k)) == sorted(P.PHASE_NAMES)
    ncuts = {}
    for name, pl in plants.items():
        (lo, hi, subs), = pl.chunks
        fixed, rows, qv, _ = _db(pl).polish_batch(pl.names(), pl.seqs(), P.THRE, pl.passes)
        # pass 0 restores the truth, one row per substitution, and the QV pass finds nothing: the later class maps are known
        assert fixed == [pl.truth[lo:hi]], name
        if pl.passes:
            assert rows[0].count("\r\n") == len(subs) and qv[0] == len(subs) * k and qv[2] == 0, (name, qv)
        else:
            # the walk stands on exactly the dips the restated walk says, one bad k-mer each
            assert qv[0] == len(P.walk_hits(pl.classes(0, 0), k)), (name, qv)
        ncuts[name] = [len(P.cuts(pl.classes(0, p), hi - lo, k, g)) for p in range(pl.passes + 1)]
        assert pl.segments(g) == sum(ncuts[name]) + pl.passes + 1
    # what each plant is there for (cuts in pass 0; later passes of the substitution plants have none: the chunks are short)
    want = {"spacing_-1": 1, "spacing_+0": 2, "spacing_+1": 2, "first_-1": 0, "first_+0": 1, "last_-1": 0, "last_+0": 1,
            "nwin_2T": 0, "nwin_2T+1": 1, "left_neighbour_legal": 1, "left_neighbour_too_close": 0,
            "nwin_2C": 0, "nwin_2C+1": 1, "attempts_8_fail": 0, "attempts_7_fail": 1}
    for name, n in want.items():
        assert ncuts[name][0] == n and sum(ncuts[name][1:]) == 0, (name, ncuts[name])
    assert ncuts["clean_cuts_3"][0] >= 3
    assert ncuts["second_attempt"][0] == ncuts["second_attempt_ref"][0] - 1 >= 1
    p0 = CELL + CELL // 2
    assert P.clean_cells(plants["second_attempt"].classes(0, 0), k, CELL)[1] == p0 + 1
    # the dips on either side of the cut taken leave it where it was, and the walk stands on them
    for name, d in (("dip_left_of_cut", CELL // 2 - 4 * k - 1), ("dip_right_of_cut", CELL // 2 + k)):
        cls = plants[name].classes(0, 0)
        assert (CELL // 2, 1) in P.cuts(cls, 2 * CELL, k, g) and P.walk_hits(cls, k)[-1] == d and cls[d] == P.BAD


def _phase_check(k, name, pl, on_stride):
    (lo, hi, _), = pl.chunks
    db = _db(pl)
    cls = pl.classes(0, 0)
    probe = int(np.nonzero(cls)[0][-1])
    hits = P.walk_hits(cls, k)
    assert (probe in hits) == on_stride, name
    wrong = {j: db.polish_batch(pl.names(), pl.seqs(prepend=j), P.THRE, 0)[2][0] for j in range(k - 1)}
    assert wrong[0] == len(hits), (name, wrong)
    if on_stride:
        # any other arrival phase gives other counters
        assert all(wrong[j] != wrong[0] for j in range(1, k - 1)), (name, wrong)
    else:
        # the one phase that would count the probe (one window later) gives other counters
        assert wrong[k - 2] != wrong[0], (name, wrong)
    # the probe sits behind the chain it is meant to test: cuts, and the segments that are clean
    cuts = P.cuts(cls, hi - lo, k, P.geometry(k))
    assert all(ch for _, ch in cuts)
    return cuts, probe


@pytest.mark.parametrize("k", P.KS)
def test_phase_probes_discriminate(k):
    for name, (pl, on) in P.phase_plants(k).items():
        cuts, probe = _phase_check(k, name, pl, on)
        assert len(cuts) == 4 and probe > cuts[1 if "one_clean" in name else 3][0] + k, name


def test_long_chain_phase_probe_discriminates():
    k = 37
    pl, on = P.phase_plants(k, long_chain=True)["behind_71_clean"]
    cuts, probe = _phase_check(k, "behind_71_clean", pl, on)
    assert len(cuts) == 72 and probe > cuts[-1][0] + k


def test_ragged_batch_plant_is_fixed_by_pass_0():
    k = 37
    pl, extra = P.ragged_batch(k)
    T = P.geometry(k)["TMIN"]
    lens = [hi - lo for lo, hi, _ in pl.chunks]
    assert 0 in lens and k + 3 in lens and 2 * T + k - 1 in lens and 2 * T + k in lens and max(lens) <= 300_000
    fixed, rows, qv, _ = _db(pl).polish_batch(pl.names(), pl.seqs(), P.THRE, pl.passes)
    assert fixed == [pl.truth[lo:hi] for lo, hi, _ in pl.chunks]
    assert rows[0].count("\r\n") == sum(len(s) for _, _, s in pl.chunks) and rows[1] == "" and qv[2] == 0
    assert pl.segments() > 3 * len(pl.chunks) + 100
    # the extra text: fix records of every kind
    _, rows, _, _ = _db(pl).polish_batch([n for n, _ in extra], [t for _, t in extra], P.THRE, pl.passes)
    assert all(any(" %s" % tag in line for line in rows[0].split("\r\n")) for tag in ("s", "i", "d-"))
