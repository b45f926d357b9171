#!/usr/bin/env python3
"""The polisher's integers, call by call, for comparing two builds of the library (GPU box):

    JASPER_AMD_LIB=other/libjasper_hip.so python tools/polish_crosscheck.py > other.jsonl
    python tools/polish_crosscheck.py > this.jsonl          # the two files must be equal

One JSON line per polishing call -- segments, respeculated, lookups, retried, the QV quadruple, the record count -- on the plants of
tests/test_gpu_polish_paths.py (the ragged batch under every setting of the rare paths, the cut and phase plants) and on bench.py's
input (the first call in one lane, the next two in three)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polish_plant as P  # noqa: E402
from jasper_amd import KmerTable, polisher  # noqa: E402

KNOBS = ("LANES", "HOST_BOOKKEEPING", "TEST_REDO", "TEST_REDO_NOROOM", "TIGHT")


def line(call, res):
    print(json.dumps(dict(call=call, segments=int(res.segments), respeculated=int(res.respeculated), lookups=int(res.lookups), retried=bool(res.retried),
                          qv=[int(x) for x in res.qv], records=int(res.n_records))), flush=True)


def polish(call, t, names, seqs, passes, **kw):
    for name in KNOBS:
        os.environ.pop("JASPER_POLISH_" + name, None)
    os.environ.update({"JASPER_POLISH_" + k: str(v) for k, v in kw.items()})
    line(call, polisher.polish_batch(t, names, seqs, P.THRE, passes)[3])
    for name in KNOBS:
        os.environ.pop("JASPER_POLISH_" + name, None)


def table_of(plant, made={}):
    key = (plant.k, id(plant.truth), tuple(plant.pieces))
    if key not in made:
        made[key] = KmerTable(plant.k, min_slots=1 << 20)
        made[key].count_bases(plant.reads())
    return made[key]


def main():
    plant, extra = P.ragged_batch(37)
    t = table_of(plant)
    names, seqs = plant.names() + [n for n, _ in extra], plant.seqs() + [s for _, s in extra]
    settings = [("ordinary", dict(LANES=1)), ("ordinary_3_lanes", dict(LANES=3)), ("host_bookkeeping", dict(LANES=1, HOST_BOOKKEEPING=1)),
                ("host_bookkeeping_3_lanes", dict(LANES=3, HOST_BOOKKEEPING=1)), ("redo_all", dict(LANES=1, TEST_REDO="all")), ("redo_0_2_4_6", dict(LANES=1, TEST_REDO="0,2,4,6")),
                ("redo_0_7", dict(LANES=1, TEST_REDO="0,7")), ("redo_1_2", dict(LANES=1, TEST_REDO="1,2")), ("redo_all_noroom", dict(LANES=1, TEST_REDO="all", TEST_REDO_NOROOM=1)),
                ("redo_0_7_noroom", dict(LANES=1, TEST_REDO="0,7", TEST_REDO_NOROOM=1)), ("redo_all_3_lanes", dict(LANES=3, TEST_REDO="all")),
                ("redo_all_tight", dict(LANES=1, TEST_REDO="all", TIGHT=1)), ("tight", dict(LANES=1, TIGHT=1))]
    for name, kw in settings:
        polish("ragged/" + name, t, names, seqs, plant.passes, **kw)
    for k in P.KS:
        plants = list(P.cut_plants(k).items()) + [(n, p) for n, (p, _) in P.phase_plants(k).items()]
        for name, pl in plants:
            polish("k%d/%s" % (k, name), table_of(pl), pl.names(), pl.seqs(), pl.passes, LANES=1)
    # bench.py's input
    import torch
    import bench as B
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    reads, _, _, d_chunks, _, _, nreads = B.build_workload(torch, dev, 0, 1, 47.0, 2)
    bt = KmerTable(B.K, min_slots=max(1 << 21, int(1.25 * int(nreads * 150 * 2.1 / 10))))
    bt.count_bases_device(reads.data_ptr(), reads.numel())
    thr = int(polisher.threshold_from_histo_rows(bt.histo_rows())[0])
    for call in range(3):
        res = None          # (a result that is still alive is brought to the host before the table's arenas are reused)
        res = bt.polish_batch_device(d_chunks[0], d_chunks[1], thr, B.PASSES, fix=True)
        line("bench/call%d" % call, res)


if __name__ == "__main__":
    main()
