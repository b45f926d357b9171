"""CPU: the host side of the duplication map -- the writers of jasper_amd/dups.py on hand-made counters and runs (formatting, NA, the
order of rows, the best_mate tie rule, the min-run filter that applies to the BED only), the flags of the driver and of kmerqc, and the
stand-alone sanitizer build of the C++ conversion of a run's mate (tools/dups_host_check.cpp).  Nothing here touches a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["ctgA", "ctgB", "ctgC"]
# (windows, valid, two_copy, deficit, multi, unplaced, sum_reads)
COUNTS = [(1000, 990, 300, 120, 7, 0, 4500), (500, 500, 300, 0, 0, 2, 9000), (80, 0, 0, 0, 0, 0, 0)]
# (seq, start, n_kmers, mate_seq, mate_start, strand, sum_reads, n_deficit)
RUNS = [(0, 10, 100, 1, 50, 0, 1500, 100), (0, 200, 100, 0, 600, 0, 1500, 10), (0, 400, 5, 1, 0, 1, 75, 5), (0, 600, 95, 0, 200, 0, 1425, 5),
        (1, 0, 5, 0, 400, 1, 75, 0), (1, 50, 100, 0, 10, 0, 3000, 0)]


def test_best_mate_and_its_tie_rule():
    from jasper_amd import dups
    # ctgA: 105 windows with ctgB (100 + 5), 195 with itself -> itself; ctgC has no run
    assert dups.best_mates(NAMES, RUNS) == [("ctgA", 195), ("ctgA", 105), (".", 0)]
    # a tie goes to the first sequence in input order, whatever the order of the runs
    tie = [(2, 0, 50, 1, 0, 0, 0, 0), (2, 100, 50, 0, 0, 1, 0, 0)]
    assert dups.best_mates(NAMES, tie)[2] == ("ctgA", 50) and dups.best_mates(NAMES, tie[::-1])[2] == ("ctgA", 50)


def test_tsv_rows_na_and_order():
    from jasper_amd import dups
    rows = dups.extended(COUNTS, NAMES, RUNS)
    txt = dups.dups_tsv_text(15, NAMES, [("before", [1020, 520, 100], rows), ("after", [1020, 0, 100], [rows[0], None, rows[2]])])
    lines = txt.split("\n")
    assert lines[0] == "#contig\tstage\tlength\twindows\tvalid\ttwo_copy\tdeficit\tmulti\tunplaced\tread_copies\tbest_mate\tbest_windows\tbest_fraction"
    assert lines[1] == "ctgA\tbefore\t1020\t1000\t990\t300\t120\t7\t0\t1.00\tctgA\t195\t0.1970"
    assert lines[2] == "ctgA\tafter\t1020\t1000\t990\t300\t120\t7\t0\t1.00\tctgA\t195\t0.1970"
    assert lines[3] == "ctgB\tbefore\t520\t500\t500\t300\t0\t0\t2\t2.00\tctgA\t105\t0.2100"
    assert lines[4] == "ctgB\tafter\t0\t0\t0\t0\t0\t0\t0\tNA\t.\t0\tNA"                       # a contig the stage does not have
    assert lines[5] == "ctgC\tbefore\t100\t80\t0\t0\t0\t0\t0\tNA\t.\t0\tNA"                    # no two-copy window, no valid window
    assert lines[7] == "*\tbefore\t1640\t1580\t1490\t600\t120\t7\t2\t1.50\t.\t300\t0.2013"
    assert lines[8] == "*\tafter\t1120\t1080\t990\t300\t120\t7\t0\t1.00\t.\t195\t0.1970"
    assert lines[9] == "" and len(lines) == 10


def test_bed_and_the_min_run_filter():
    from jasper_amd import dups
    k = 21
    bed = dups.bed_text(k, 15, NAMES, RUNS, 1).split("\n")
    assert bed[0] == "ctgA\t10\t130\tctgB\t50\t170\t+\t100\t1.00\t1.0000"
    assert bed[2] == "ctgA\t400\t425\tctgB\t0\t25\t-\t5\t1.00\t1.0000"
    assert bed[5] == "ctgB\t50\t170\tctgA\t10\t130\t+\t100\t2.00\t0.0000" and len(bed) == 7
    short = dups.bed_text(k, 15, NAMES, RUNS, 95)
    assert len(short.split("\n")) == 5 and "\t-\t" not in short and len(dups.listed(RUNS, 95)) == 4      # the two runs of 5 are gone
    assert len(dups.listed(RUNS, 96)) == 3
    assert dups.bed_text(k, 15, NAMES, [], 1) == ""
    # numpy records are read by field name
    import numpy as np
    from jasper_amd.table import DUPRUN_DTYPE
    rec = np.zeros(1, dtype=DUPRUN_DTYPE)
    rec[0] = (10, 50, 100, 1500, 100, 0, 1, 0, 0)
    assert dups.bed_text(k, 15, NAMES, rec, 1) == bed[0] + "\n"


def test_pairs_count_runs_of_every_length():
    from jasper_amd import dups
    txt = dups.pairs_tsv_text(15, [("before", NAMES, RUNS), ("after", NAMES, RUNS[:1])])
    assert txt.split("\n") == ["#stage\tcontig\tmate\tstrand\truns\twindows\tdeficit\tread_copies",
                               "before\tctgA\tctgA\t+\t2\t195\t15\t1.00",
                               "before\tctgA\tctgB\t+\t1\t100\t100\t1.00",
                               "before\tctgA\tctgB\t-\t1\t5\t5\t1.00",                        # (shorter than any min_run but 1: listed all the same)
                               "before\tctgB\tctgA\t+\t1\t100\t0\t2.00",
                               "before\tctgB\tctgA\t-\t1\t5\t0\t1.00",
                               "after\tctgA\tctgB\t+\t1\t100\t100\t1.00", ""]
    assert dups.pairs_tsv_text(15, [("asm", NAMES, [])]) == dups.PAIRS_HEADER


def test_log_text():
    from jasper_amd import dups
    rows = dups.extended(COUNTS, NAMES, RUNS)
    assert dups.stage_log_text(rows, 4) == "600 two-copy, 120 deficit, 7 multi and 2 unplaced windows, 4 runs listed"
    assert dups.stage_log_text([rows[0], None], 0) == "300 two-copy, 120 deficit, 7 multi and 0 unplaced windows, 0 runs listed"


def test_flags(capsys):
    from jasper_amd import cli, kmerqc
    o = cli.parse_args(["-a", "x/asm.fa", "--dups", "--peak", "31", "--dups-min-run", "1"])
    assert o.dups and o.dups_min_run == "1" and not o.copies
    assert cli.dups_flags(o.dups, o.peak, o.dups_min_run) == (31, 1)
    assert cli.dups_flags(True, None, None) == (None, None) and cli.dups_flags(False, "31", None) == (None, None)
    assert not cli.parse_args(["-a", "x/asm.fa"]).dups
    a = kmerqc.parse_args(["-a", "asm.fa", "-r", "r.fq", "--dups", "--dups-min-run", "3"])
    assert a["dups"] and a["dups_min_run"] == "3" and not a["copies"]
    for args, msg in (((False, None, "5"), "give --dups as well"), ((True, None, "0"), "--dups-min-run takes an integer of at least 1"),
                      ((True, None, "x"), "--dups-min-run takes an integer of at least 1"), ((True, "0", None), "--peak")):
        with pytest.raises(SystemExit) as e:
            cli.dups_flags(*args)
        assert e.value.code == 1
        out = capsys.readouterr()
        assert msg in out.out + out.err


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/dups_host_check.cpp: the encoding, the sequence of a global position across empty sequences and boundaries, the `-` flip
    and the refusals of jasper_amd/csrc/dups_host.hpp as a stand-alone program built with -fsanitize=address,undefined"""
    import shutil
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "dups_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "dups_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
