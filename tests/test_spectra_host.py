"""CPU: jasper_amd/spectra.py -- the numbers derived from a copy-number spectrum and the two file formats -- on matrices written
out here, and the option parsers' --spectra flag.  No GPU, no library call."""
import pytest

from jasper_amd import cli, kmerqc, spectra

ROWS, COLS = 6, 10002


def matrix(cells):
    """{(row, column): value} -> 6 x 10002 lists"""
    S = [[0] * COLS for _ in range(ROWS)]
    for (m, c), v in cells.items():
        S[m][c] = v
    return S


# reads: 7 k-mers seen once (5 of them in no assembly copy), 40 seen 30 times, 3 seen 10001 times or more; assembly-only: 4 + 1
SMALL = {(0, 1): 5, (0, 30): 2, (1, 1): 2, (1, 30): 35, (2, 30): 2, (5, 30): 1, (3, 10001): 3, (1, 0): 4, (5, 0): 1, (4, 2047): 6, (0, 2048): 1}


def test_shape_constants_and_labels():
    assert (spectra.ROWS, spectra.COLS) == (ROWS, COLS)
    assert spectra.ROW_LABELS == ("0", "1", "2", "3", "4", ">4")
    with pytest.raises(ValueError):
        spectra.cells_of([[0] * COLS] * 5)


def test_derived_numbers():
    S = matrix(SMALL)
    # threshold 1: every k-mer of the reads is solid
    assert spectra.derived(S, 1) == (5 + 2 + 2 + 35 + 2 + 1 + 3 + 6 + 1, 2 + 35 + 2 + 1 + 3 + 6, 2 + 35 + 2 + 1 + 3 + 4 + 1 + 6, 5)
    # threshold 2 drops column 1 from solid and found, not from the assembly's distinct k-mers
    assert spectra.derived(S, 2) == (2 + 35 + 2 + 1 + 3 + 6 + 1, 35 + 2 + 1 + 3 + 6, 54, 5)
    assert spectra.derived(S, 31) == (3 + 6 + 1, 3 + 6, 54, 5)
    assert spectra.derived(S, 2049) == (3, 3, 54, 5)
    assert spectra.derived(S, 10001) == (3, 3, 54, 5)
    assert spectra.derived(S, 10002) == (0, 0, 54, 5)
    # a k-mer the reads do not have is never solid: a threshold below 1 counts as 1
    assert spectra.derived(S, 0) == spectra.derived(S, 1)


def test_derived_numbers_take_numpy_and_objects_with_cells():
    import numpy as np
    S = np.array(matrix(SMALL), dtype=np.uint64)

    class Spec:
        cells = S
    assert spectra.derived(S, 2) == spectra.derived(matrix(SMALL), 2) == spectra.derived(Spec(), 2)
    assert all(isinstance(v, int) for v in spectra.derived(S, 2))
    big = matrix({(1, 5): 2**63 + 5, (0, 5): 2**63})          # sums beyond 64 bits stay exact
    assert spectra.derived(np.array(big, dtype=np.uint64), 1)[0] == 2**64 + 5


def test_completeness_percentage():
    assert spectra.completeness_pct(0, 0) == "NA"
    assert spectra.completeness_pct(1, 3) == "33.3333"
    assert spectra.completeness_pct(2, 3) == "66.6667"
    assert spectra.completeness_pct(3, 3) == "100.0000"
    assert spectra.completeness_pct(0, 7) == "0.0000"
    assert spectra.completeness_pct(5526, 5957) == "92.7648"


def test_spectra_cn_text_bytes():
    want = ("#copies\tread_count\tkmers\n"
            "0\t1\t5\n" "0\t30\t2\n" "0\t2048\t1\n"
            "1\t0\t4\n" "1\t1\t2\n" "1\t30\t35\n"
            "2\t30\t2\n"
            "3\t10001\t3\n"
            "4\t2047\t6\n"
            ">4\t0\t1\n" ">4\t30\t1\n")
    assert spectra.spectra_cn_text(matrix(SMALL)) == want
    assert spectra.spectra_cn_text(matrix({})) == "#copies\tread_count\tkmers\n"


def test_completeness_text_bytes():
    S = matrix(SMALL)
    rows = [spectra.completeness_row("before", S, 2), spectra.completeness_row("after", matrix({(0, 1): 9, (2, 0): 3}), 2)]
    assert rows[0] == ("before", 2, 50, 47, 54, 5)
    want = ("#stage\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tasm_distinct\tasm_only\n"
            "before\t25\t2\t50\t47\t94.0000\t54\t5\n"
            "after\t25\t2\t0\t0\tNA\t3\t3\n")
    assert spectra.completeness_text(25, rows) == want
    assert spectra.log_text(rows[0]) == "k-mer completeness = 94.0000 % (47 of 50 solid k-mers, threshold 2); 5 assembly-only k-mers"
    assert spectra.log_text(rows[1]) == "k-mer completeness = NA (0 of 0 solid k-mers, threshold 2); 3 assembly-only k-mers"


def test_files_are_written_through_a_tmp_name(tmp_path):
    p = tmp_path / "x.spectra_cn.tsv"
    spectra.write_atomic(str(p), spectra.spectra_cn_text(matrix(SMALL)))
    assert p.read_text() == spectra.spectra_cn_text(matrix(SMALL))
    assert [f.name for f in tmp_path.iterdir()] == ["x.spectra_cn.tsv"]
    from jasper_amd import report
    assert spectra.write_atomic is report.write_atomic


def test_cli_parser_takes_spectra(capsys):
    with_flag = cli.parse_args(["-a", "x/asm.fa", "--spectra", "-k", "25"])
    without = cli.parse_args(["-a", "x/asm.fa", "-k", "25"])
    assert with_flag.spectra is True and without.spectra is False
    a, b = dict(vars(with_flag)), dict(vars(without))
    del a["spectra"], b["spectra"]
    assert a == b and b["report"] is False and b["kmer"] == "25" and b["query_fn"] == "asm.fa"
    both = cli.parse_args(["--report", "--spectra"])
    assert both.report and both.spectra
    assert cli.parse_args(["--report"]).spectra is False
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["-a", "asm.fa", "--spectrum"])
    assert e.value.code == 1
    assert capsys.readouterr().out == "Unknown option --spectrum\n"


def test_kmerqc_parser_takes_spectra(capsys):
    args = ["-a", "asm.fa", "-j", "db.jf", "--threshold", "4", "-o", "out/p"]
    without = kmerqc.parse_args(args)
    assert without["spectra"] is False
    for argv in (["--spectra"] + args, args + ["--spectra"], args[:2] + ["--spectra"] + args[2:]):
        got = kmerqc.parse_args(argv)
        assert got["spectra"] is True
        assert {k: v for k, v in got.items() if k != "spectra"} == {k: v for k, v in without.items() if k != "spectra"}
    assert (without["asm"], without["jf"], without["reads"], without["threshold"], without["prefix"], without["k"], without["device"]) == \
        ("asm.fa", "db.jf", None, "4", "out/p", "37", 0)
    with pytest.raises(SystemExit) as e:
        kmerqc.parse_args(["-a", "asm.fa", "--spectra", "--polish"])
    assert e.value.code == 1 and "Unknown option --polish" in capsys.readouterr().out
