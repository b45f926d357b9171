"""CPU: the writers of the dense k-mer report (jasper_amd/report.py) on hand-made counters and runs, the --report flag of the
drop-in CLI, and the stand-alone evaluator's argument parser.  No GPU call anywhere here."""
import math

import pytest

from jasper_amd import report


def test_core_formula_at_one_k_and_k_plus_one():
    k = 5
    names = ["c0", "c1"]
    runs = [(0, 10, 1, 1, 0), (0, 40, k, 2, 1), (1, 7, k + 1, 0, 3), (1, 100, 30, 30, 0)]
    lines = report.bed_text(k, names, runs).splitlines()
    assert lines == [
        # contig start end n_kmers n_absent min_count core_start core_end
        "c0\t10\t15\t1\t1\t0\t10\t15",          # one window: the core is the window itself
        "c0\t40\t49\t5\t2\t1\t44\t45",          # k windows: one base is in all of them
        "c1\t7\t17\t6\t0\t3\t7\t7",             # k + 1 windows: no base is in all of them
        "c1\t100\t134\t30\t30\t0\t100\t100",
    ]
    # the core really is the intersection of the windows
    for _, start, nk, _, _ in runs:
        common = set(range(start, start + k))
        for i in range(start, start + nk):
            common &= set(range(i, i + k))
        f = report.bed_text(k, names, [(0, start, nk, 0, 0)]).split()
        cs, ce = int(f[6]), int(f[7])
        assert set(range(cs, ce)) == common
        assert int(f[2]) == start + nk + k - 1


def test_bed_accepts_the_numpy_run_array():
    np = pytest.importorskip("numpy")
    from jasper_amd.table import KMERRUN_DTYPE
    a = np.zeros(1, dtype=KMERRUN_DTYPE)
    a[0] = (3_000_000_000, 2, 1, 0, 4)          # (start, n_kmers, n_absent, seq, min_count): 64-bit positions
    assert report.bed_text(31, ["big"], a) == "big\t3000000000\t3000000032\t2\t1\t4\t3000000001\t3000000031\n"


def test_qv_text_inf_na_and_value():
    assert report.qv_text(0, 100, 25) == "inf"
    assert report.qv_text(0, 0, 25) == "NA"
    assert report.qv_text(5, 0, 25) == "NA"
    want = -10 * math.log10(1 - (1 - 450 / 5976) ** (1 / 25))
    assert report.qv_text(450, 5976, 25) == "%.4f" % want
    assert report.qv_text(7, 7, 31) == "0.0000"                 # every window counted against it: error rate 1


def test_tsv_row_order_star_rows_and_a_missing_polished_contig():
    k = 25
    names = ["a", "b", "c"]
    before = [(100, 100, 10, 5), (0, 0, 0, 0), (50, 40, 0, 0)]
    polished_names, polished_len, polished_counts = ["c", "a"], [74, 125], [(50, 50, 0, 0), (101, 101, 2, 0)]
    len1, cnt1 = report.align(names, polished_names, polished_len, polished_counts)
    assert len1 == [125, 0, 74] and cnt1 == [(101, 101, 2, 0), None, (50, 50, 0, 0)]
    txt = report.qv_tsv_text(k, names, [("before", [124, 10, 74], before), ("after", len1, cnt1)])
    rows = [ln.split("\t") for ln in txt.splitlines()]
    assert txt.endswith("\n") and rows[0] == ["#contig", "stage", "length", "windows", "valid", "unreliable", "absent", "QV_unreliable", "QV_absent"]
    assert [(r[0], r[1]) for r in rows[1:]] == [("a", "before"), ("a", "after"), ("b", "before"), ("b", "after"), ("c", "before"), ("c", "after"),
                                                ("*", "before"), ("*", "after")]
    assert rows[1][2:] == ["124", "100", "100", "10", "5", report.qv_text(10, 100, k), report.qv_text(5, 100, k)]
    assert rows[3][2:] == ["10", "0", "0", "0", "0", "NA", "NA"]                 # shorter than k: zeros
    assert rows[4] == ["b", "after", "0", "0", "0", "0", "0", "NA", "NA"]        # missing from the polished FASTA
    assert rows[5][2:] == ["74", "50", "40", "0", "0", "inf", "inf"]
    assert rows[7] == ["*", "before", "208", "150", "140", "10", "5", report.qv_text(10, 140, k), report.qv_text(5, 140, k)]
    assert rows[8] == ["*", "after", "199", "151", "151", "2", "0", report.qv_text(2, 151, k), "inf"]


def test_contig_name_is_the_first_token_without_the_mark():
    assert report.contig_name(">ctg1 len=5 cov=3") == "ctg1"
    assert report.contig_name(">ctg1") == "ctg1"
    assert report.contig_name("ctg2\tx") == "ctg2"


def test_write_atomic_leaves_no_tmp(tmp_path):
    p = str(tmp_path / "x.tsv")
    report.write_atomic(p, "a\n")
    assert open(p).read() == "a\n" and [f.name for f in tmp_path.iterdir()] == ["x.tsv"]


def test_cli_accepts_report_and_still_refuses_unknown_flags(capsys):
    from jasper_amd import cli
    o = cli.parse_args(["-a", "x/asm.fa", "--report", "-k", "25"])
    assert o.report is True and o.kmer == "25" and o.query_fn == "asm.fa"
    assert cli.parse_args(["-a", "asm.fa"]).report is False
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["-a", "asm.fa", "--reports"])
    assert e.value.code == 1
    assert capsys.readouterr().out == "Unknown option --reports\n"


def test_kmerqc_arguments(capsys):
    from jasper_amd import kmerqc
    a = kmerqc.parse_args(["-a", "asm.fa", "-j", "db.jf", "--threshold", "4", "-o", "out/p"])
    assert (a["asm"], a["jf"], a["reads"], a["threshold"], a["prefix"], a["k"]) == ("asm.fa", "db.jf", None, "4", "out/p", "37")
    with pytest.raises(SystemExit) as e:
        kmerqc.parse_args(["-a", "asm.fa", "--polish"])
    assert e.value.code == 1 and "Unknown option --polish" in capsys.readouterr().out


def test_report_symbols_are_declared_bound_and_exported():
    """(tests/test_lib_abi.py demands that header, binding table and library agree; this names the report's calls)"""
    from jasper_amd import _lib
    import test_lib_abi as abi
    want = {"jasper_kmer_report", "jasper_kmer_report_device", "jasper_report_num_seqs", "jasper_report_counts", "jasper_report_runs",
            "jasper_report_seconds", "jasper_report_free"}
    assert want <= set(abi.declared_symbols()) and want <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for name in want:
        assert hasattr(L, name)
    assert L.jasper_report_tile_windows() == 4096
