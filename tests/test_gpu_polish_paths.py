"""GPU: the polishing walk's rare paths on planted inputs (tests/polish_plant.py) -- the host's own bookkeeping against the device's,
the redo of chunks whose speculation failed (forced: JASPER_POLISH_TEST_REDO), where the cuts fall, and what arrival a chain of
segments hands down.  Every expectation is fixed without a GPU (tests/test_polish_cuts_host.py); every comparison is exact equality
with the oracle."""
import contextlib
import os
import sys

import pytest

import polish_plant as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = "Contig Base_coord Original Mutation\r\n"
KNOBS = ("JASPER_POLISH_LANES", "JASPER_POLISH_HOST_BOOKKEEPING", "JASPER_POLISH_TEST_REDO", "JASPER_POLISH_TEST_REDO_NOROOM",
         "JASPER_POLISH_TIGHT")


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


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


@pytest.fixture(scope="module")
def world(KT, O):
    """(table, oracle map) of a plant's reads; plants with the same reads share them"""
    made = {}

    def get(plant):
        key = (plant.k, id(plant.truth), tuple(plant.pieces))
        if key not in made:
            reads = plant.reads()
            t = KT(plant.k, min_slots=1 << 20)
            t.count_bases(reads)
            db = O.OracleDB(plant.k)
            db.count_bases(reads)
            made[key] = (t, db)
        return made[key]
    yield get
    for t, _ in made.values():
        t.close()


def polish(t, names, seqs, passes, **kw):
    from jasper_amd import polisher
    with knobs(**kw):
        fixed, rows, qv, res = polisher.polish_batch(t, names, seqs, P.THRE, passes)
    return fixed, [polisher.fix_csv_text(r) for r in rows], qv, res


def everything(res, n):
    return (res.seqs, res.records, res.qv, [res.qv_chunk(i) for i in range(n)], res.segments, res.lookups)


# ---- a. and b.: the host's bookkeeping, the redo ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged(world):
    """the ragged batch, the oracle's answer and the ordinary run's (one lane, the device's bookkeeping)"""
    plant, extra = P.ragged_batch(37)
    t, db = world(plant)
    names = plant.names() + [n for n, _ in extra]
    seqs = plant.seqs() + [s for _, s in extra]
    fixed_o, rows_o, qv_o, _ = db.polish_batch(names, seqs, P.THRE, plant.passes)
    fixed, rows, qv, res = polish(t, names, seqs, plant.passes, LANES=1)
    print("ordinary run: segments %d, respeculated %d" % (res.segments, res.respeculated))
    assert fixed == fixed_o and qv == qv_o and rows == [HEADER + r for r in rows_o]
    assert any(r["kind"] == "x" for r in res.records)                       # (records with aux bytes: aux_off matters)
    # the plant's chunks cut where the restated rule says; the extra text has one chunk with segments of its own
    lone = polish(t, names[:-1], seqs[:-1], plant.passes, LANES=1)[3]
    assert lone.segments == plant.segments() and res.segments > lone.segments
    return dict(t=t, names=names, seqs=seqs, passes=plant.passes, oracle=(fixed_o, [HEADER + r for r in rows_o], qv_o), res=res)


@pytest.mark.parametrize("lanes", [1, 3])
def test_host_bookkeeping_equals_device_bookkeeping(ragged, lanes):
    n = len(ragged["seqs"])
    fixed, rows, qv, res = polish(ragged["t"], ragged["names"], ragged["seqs"], ragged["passes"], LANES=lanes, HOST_BOOKKEEPING=1)
    assert (fixed, rows, qv) == ragged["oracle"]
    assert everything(res, n) == everything(ragged["res"], n)
    assert res.respeculated == ragged["res"].respeculated
    if lanes > 1:                       # the device's bookkeeping in lanes as well
        _, _, _, dev = polish(ragged["t"], ragged["names"], ragged["seqs"], ragged["passes"], LANES=lanes)
        assert everything(dev, n) == everything(ragged["res"], n)


REDO = {"all": None, "every_second": (0, 2, 4, 6), "first_and_last": (0, 7), "empty_and_tiny": (1, 2)}


def _check_redo(ragged, listed, **kw):
    n = len(ragged["seqs"])
    assert n == 8 and len(ragged["seqs"][2]) == 0 and len(ragged["seqs"][1]) == 37 + 3
    fixed, rows, qv, res = polish(ragged["t"], ragged["names"], ragged["seqs"], ragged["passes"],
                                  TEST_REDO="all" if listed is None else ",".join(map(str, listed)), **kw)
    assert (fixed, rows, qv) == ragged["oracle"]
    want = ragged["res"]
    assert (res.seqs, res.records, res.qv, [res.qv_chunk(i) for i in range(n)]) == (want.seqs, want.records, want.qv, [want.qv_chunk(i) for i in range(n)])
    assert want.respeculated == 0 and res.respeculated == (ragged["passes"] + 1) * (n if listed is None else len(listed))
    # the accounting counts the segments of a pass's FIRST attempt (R.n_segments += the table that was walked first), a redo
    # adds nothing: the same text is cut in the same places in every pass, so the sum is the ordinary run's
    assert res.segments == want.segments
    return res


@pytest.mark.parametrize("noroom", [False, True])
@pytest.mark.parametrize("which", list(REDO))
def test_forced_redo(ragged, which, noroom):
    _check_redo(ragged, REDO[which], LANES=1, **({"TEST_REDO_NOROOM": 1} if noroom else {}))


def test_forced_redo_of_all_in_three_lanes(ragged):
    _check_redo(ragged, None, LANES=3)


def test_forced_redo_of_all_when_the_first_attempt_runs_out_of_room(ragged):
    _check_redo(ragged, None, LANES=1, TIGHT=1)


SETTINGS = {"host_bookkeeping": dict(HOST_BOOKKEEPING=1), "redo_all": dict(TEST_REDO="all"),
            "redo_all_noroom": dict(TEST_REDO="all", TEST_REDO_NOROOM=1)}


def _fuzz(seeds, setting, tmp_path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from jasper_amd import KmerTable, polisher
    from oracle import oracle as O
    import make_golden as G
    import fuzz_vs_reference as F
    from test_gpu_fuzz import _one
    with knobs(**SETTINGS[setting]):
        for seed in seeds:
            _one(seed, KmerTable, polisher, O, G, F, tmp_path)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_fuzz_cases_on_the_rare_paths(hip, tmp_path, setting):
    _fuzz(range(5000, 5040), setting, tmp_path)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_seed_995395_on_the_rare_paths(hip, tmp_path, setting):
    """the case of round 5's open observation, once under each setting"""
    _fuzz([995395], setting, tmp_path)


# ---- c.: where the cuts fall, what a chain hands down ---------------------------------------------------------------------------

def _check_plant(world, plant):
    t, db = world(plant)
    names, seqs = plant.names(), plant.seqs()
    fixed_o, rows_o, qv_o, _ = db.polish_batch(names, seqs, P.THRE, plant.passes)
    fixed, rows, qv, res = polish(t, names, seqs, plant.passes, LANES=1)
    print("%s k=%d: segments %d (restated %d), respeculated %d, qv %s (oracle %s)" % (plant.name, plant.k, res.segments, plant.segments(),
                                                                                     res.respeculated, qv, qv_o))
    assert res.segments == plant.segments()
    assert fixed == fixed_o and qv == qv_o and rows == [HEADER + r for r in rows_o]
    return res


@pytest.fixture(scope="module")
def cut_plants():
    return {k: P.cut_plants(k) for k in P.KS}


@pytest.fixture(scope="module")
def phase_plants():
    return {k: P.phase_plants(k) for k in P.KS}


@pytest.mark.parametrize("name", P.CUT_NAMES)
@pytest.mark.parametrize("k", P.KS)
def test_cuts_fall_where_the_rule_says(world, cut_plants, k, name):
    _check_plant(world, cut_plants[k][name])


@pytest.mark.parametrize("name", P.PHASE_NAMES)
@pytest.mark.parametrize("k", P.KS)
def test_arrival_phase_down_a_chain(world, phase_plants, k, name):
    plant, on_stride = phase_plants[k][name]
    res = _check_plant(world, plant)
    assert res.qv[0] == len(plant.dips) - (0 if on_stride else 1)


def test_arrival_phase_behind_71_clean_segments(world):
    """the look-back past clean segments goes 64 at a time: a chain longer than that"""
    plant, on_stride = P.phase_plants(37, long_chain=True)["behind_71_clean"]
    res = _check_plant(world, plant)
    assert res.segments >= 66 and on_stride and res.qv[0] == 1
