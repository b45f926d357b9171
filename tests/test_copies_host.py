"""CPU: jasper_amd/copies.py -- the single-copy peak of a histogram and the texts of `*.copies.tsv` / `*.copies*.bed` for hand-made
counters and runs -- and the parsers' new flags.  The expected texts are written out here by hand from the formats in README.md."""
import numpy as np
import pytest

from jasper_amd import cli, copies, kmerqc, report


def histo(bins):
    h = [0] * 10002
    for c, n in bins.items():
        h[c] = n
    return h


def test_peak_from_histogram():
    h = histo({1: 9000, 2: 500, 3: 100, 4: 20, 5: 40, 29: 700, 30: 900, 31: 900, 32: 650, 60: 80, 10001: 5000})
    assert copies.peak_from_histogram(h, 5) == 30                      # a tie: the smallest count wins
    assert copies.peak_from_histogram(h, 0) == 30 and copies.peak_from_histogram(h, 1) == 30      # bin 1 is never the peak
    assert copies.peak_from_histogram(h, 31) == 31
    assert copies.peak_from_histogram(h, 32) == 32 and copies.peak_from_histogram(h, 33) == 60    # thre above the peak: the next mode
    assert copies.peak_from_histogram(h, 61) is None                   # bin 10001 is "that count or more": never the peak
    assert copies.peak_from_histogram(h, 20000) is None
    assert copies.peak_from_histogram(histo({}), 0) is None and copies.peak_from_histogram(histo({1: 7, 10001: 3}), 0) is None
    assert copies.peak_from_histogram(histo({2: 1}), 0) == 2 and copies.peak_from_histogram(histo({10000: 1}), 5) == 10000
    assert copies.peak_from_histogram(np.array(h, dtype=np.uint64), 5) == 30


def test_histogram_from_rows():
    h = copies.histogram_from_rows([(1, 10), ("2", "5"), (10001, 3), ["30", "7"]])
    assert len(h) == 10002 and (h[1], h[2], h[30], h[10001]) == (10, 5, 7, 3) and sum(h) == 25
    assert copies.peak_from_histogram(h, 0) == 30


NAMES = ["ctg1", "ctg2", "ctg3"]
# (windows, valid, excess, deficit, sum_reads, sum_asm)
BEFORE = [(1000, 990, 100, 0, 59400, 990), (500, 500, 0, 480, 7500, 1000), (64, 0, 0, 0, 0, 0)]
AFTER = [(1001, 1001, 90, 1, 30030, 1001), None, (64, 10, 0, 0, 300, 0)]


def test_tsv_text():
    text = copies.copies_tsv_text(30, NAMES, [("before", [1024, 524, 88], BEFORE), ("after", [1025, 0, 88], AFTER)])
    want = ("#contig\tstage\tlength\twindows\tvalid\texcess\tdeficit\tsum_reads\tsum_asm\tdepth\tpeak\n"
            "ctg1\tbefore\t1024\t1000\t990\t100\t0\t59400\t990\t2.0000\t30\n"
            "ctg1\tafter\t1025\t1001\t1001\t90\t1\t30030\t1001\t1.0000\t30\n"
            "ctg2\tbefore\t524\t500\t500\t0\t480\t7500\t1000\t0.2500\t30\n"
            "ctg2\tafter\t0\t0\t0\t0\t0\t0\t0\tNA\t30\n"                      # a contig the polished FASTA lacks
            "ctg3\tbefore\t88\t64\t0\t0\t0\t0\t0\tNA\t30\n"
            "ctg3\tafter\t88\t64\t10\t0\t0\t300\t0\tNA\t30\n"                 # valid windows, none of them in the assembly's table
            "*\tbefore\t1636\t1564\t1490\t100\t480\t66900\t1990\t1.1206\t30\n"
            "*\tafter\t1113\t1065\t1011\t90\t1\t30330\t1001\t1.0100\t30\n")
    assert text == want
    one = copies.copies_tsv_text(7, ["a"], [("asm", [40], [(10, 10, 1, 2, 35, 10)])])
    assert one.splitlines()[1:] == ["a\tasm\t40\t10\t10\t1\t2\t35\t10\t0.5000\t7", "*\tasm\t40\t10\t10\t1\t2\t35\t10\t0.5000\t7"]
    assert copies.totals(AFTER) == (1065, 1011, 90, 1, 30330, 1001)


RUNS = [(0, 10, 40, 1, 2400, 40), (0, 50, 1, 2, 3, 4), (1, 0, 480, 2, 7200, 960), (2, 7, 24, 1, 1000, 0)]


def test_bed_text_min_run_and_end():
    k = 25
    every = copies.bed_text(k, 30, NAMES, RUNS, 1)
    assert every == ("ctg1\t10\t74\texcess\t40\t60.00\t1.00\t2.00\n"            # end = start + n_kmers + k - 1
                     "ctg1\t50\t75\tdeficit\t1\t3.00\t4.00\t0.10\n"            # touches the run before it
                     "ctg2\t0\t504\tdeficit\t480\t15.00\t2.00\t0.50\n"
                     "ctg3\t7\t55\texcess\t24\t41.67\t0.00\t1.39\n")
    assert copies.bed_text(k, 30, NAMES, RUNS) == every                   # the function's default lists every run
    assert copies.bed_text(k, 30, NAMES, RUNS, 25) == "".join(every.splitlines(True)[i] for i in (0, 2))
    assert copies.bed_text(k, 30, NAMES, RUNS, 24) == "".join(every.splitlines(True)[i] for i in (0, 2, 3))
    assert copies.bed_text(k, 30, NAMES, RUNS, 481) == "" and copies.bed_text(k, 30, NAMES, [], 1) == ""
    assert [r[:3] for r in copies.listed(RUNS, 40)] == [(0, 10, 40), (1, 0, 480)]
    # the structured array of a CopyReport gives the same text
    from jasper_amd.table import COPYRUN_DTYPE
    arr = np.zeros(len(RUNS), dtype=COPYRUN_DTYPE)
    for i, (seq, start, nk, kind, sr, sa) in enumerate(RUNS):
        arr[i] = (start, nk, sr, sa, seq, kind)
    assert arr.itemsize == 40 and copies.bed_text(k, 30, NAMES, arr, 1) == every


def test_a_contig_missing_after_polishing():
    names1 = ["ctg3", "ctg1"]
    len1, cnt1 = [88, 1025], [AFTER[2], AFTER[0]]
    len1a, cnt1a = copies.align(NAMES, names1, len1, cnt1)
    assert (len1a, cnt1a) == ([1025, 0, 88], AFTER) and copies.align is report.align
    text = copies.copies_tsv_text(30, NAMES, [("before", [1024, 524, 88], BEFORE), ("after", len1a, cnt1a)])
    assert "ctg2\tafter\t0\t0\t0\t0\t0\t0\t0\tNA\t30\n" in text
    assert copies.stage_log_text(cnt1a, 3) == "90 excess and 1 deficit windows, 3 runs listed"
    assert copies.stage_log_text(BEFORE, 0) == "100 excess and 480 deficit windows, 0 runs listed"


def test_files_are_written_through_a_tmp_name(tmp_path):
    p = tmp_path / "x.copies.bed"
    copies.write_atomic(str(p), copies.bed_text(25, 30, NAMES, RUNS, 1))
    assert p.read_text() == copies.bed_text(25, 30, NAMES, RUNS, 1)
    assert [f.name for f in tmp_path.iterdir()] == ["x.copies.bed"]
    assert copies.write_atomic is report.write_atomic


def test_cli_parser_takes_the_flags(capsys):
    without = cli.parse_args(["-a", "x/asm.fa", "-k", "25"])
    assert (without.copies, without.peak, without.copies_min_run) == (False, None, None)
    o = cli.parse_args(["-a", "x/asm.fa", "--copies", "--peak", "31", "-k", "25", "--copies-min-run", "1"])
    assert (o.copies, o.peak, o.copies_min_run) == (True, "31", "1")
    a, b = dict(vars(o)), dict(vars(without))
    for key in ("copies", "peak", "copies_min_run"):
        del a[key], b[key]
    assert a == b and b["kmer"] == "25" and b["spectra"] is False and b["report"] is False
    both = cli.parse_args(["--copies", "--spectra", "--report"])
    assert both.copies and both.spectra and both.report and both.peak is None
    assert cli.copies_flags(None, None) == (None, None) and cli.copies_flags("31", "1") == (31, 1)
    for bad in (("0", None), ("x", None), (None, "0"), ("-3", "5"), (str(2**32), None)):
        with pytest.raises(SystemExit) as e:
            cli.copies_flags(*bad)
        assert e.value.code == 1
    assert "--peak" in capsys.readouterr().err
    assert cli.copies_peak(17, [0] * 10002, 5) == 17 and cli.copies_peak(None, [0] * 30 + [4] + [0] * 9971, 5) == 30
    with pytest.raises(SystemExit) as e:
        cli.copies_peak(None, [0] * 10002, 5)
    assert e.value.code == 1 and "--peak" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--copy"])


def test_kmerqc_parser_takes_the_flags():
    args = ["-a", "asm.fa", "-j", "db.jf", "--threshold", "4", "-o", "out/p"]
    without = kmerqc.parse_args(args)
    assert (without["copies"], without["peak"], without["min_run"], without["spectra"]) == (False, None, None, False)
    got = kmerqc.parse_args(["--copies"] + args + ["--peak", "28", "--copies-min-run", "3"])
    assert (got["copies"], got["peak"], got["min_run"], got["spectra"]) == (True, "28", "3", False)
    assert {k: v for k, v in got.items() if k not in ("copies", "peak", "min_run")} == {k: v for k, v in without.items() if k not in ("copies", "peak", "min_run")}
    assert kmerqc.parse_args(args + ["--copies", "--spectra"])["spectra"] is True
    with pytest.raises(SystemExit) as e:
        kmerqc.parse_args(args + ["--peak"])
    assert e.value.code == 1
