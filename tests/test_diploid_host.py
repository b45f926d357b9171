"""CPU: jasper_amd/diploid.py -- the numbers derived from a pair spectrum and the four file formats of kmerqc --alt -- on hand-written
matrices and runs; kmerqc's parsing and early checks of --alt; and, with a recording fake table, how often the -a assembly is counted."""
import os

import numpy as np
import pytest

from jasper_amd import cli, diploid, extensions, kmerqc, report


def matrix(cells):
    """{(row, column): kmers} -> 4 x 10002"""
    P = np.zeros((4, 10002), dtype=np.uint64)
    for (j, c), v in cells.items():
        P[j, c] = v
    return P


# reads_only: 7 at count 1, 20 at count 30; asm_only: 2 not in the reads, 1 at count 1, 3 at count 30; alt_only: 4 at count 2, 5 at 10001;
# shared: 1 not in the reads, 100 at count 30, 6 at count 10001
SMALL = {(0, 1): 7, (0, 30): 20, (1, 0): 2, (1, 1): 1, (1, 30): 3, (2, 2): 4, (2, 10001): 5, (3, 0): 1, (3, 30): 100, (3, 10001): 6}


def test_spectra_asm_text_lists_the_non_zero_cells_by_class_and_column():
    assert diploid.spectra_asm_text(matrix(SMALL)) == (
        "#class\tread_count\tkmers\n"
        "reads_only\t1\t7\nreads_only\t30\t20\n"
        "asm_only\t0\t2\nasm_only\t1\t1\nasm_only\t30\t3\n"
        "alt_only\t2\t4\nalt_only\t10001\t5\n"
        "shared\t0\t1\nshared\t30\t100\nshared\t10001\t6\n")
    no_alt = {key: v for key, v in SMALL.items() if key[0] != 2}                  # an empty class has no line
    assert "alt_only" not in diploid.spectra_asm_text(matrix(no_alt))
    assert diploid.spectra_asm_text(np.zeros((4, 10002), dtype=np.uint64)) == diploid.SPECTRA_HEADER
    assert diploid.spectra_asm_text([list(r) for r in matrix(SMALL)]) == diploid.spectra_asm_text(matrix(SMALL))
    with pytest.raises(ValueError):
        diploid.spectra_asm_text(np.zeros((6, 10002), dtype=np.uint64))           # (the copy-number spectrum is another matrix)


def test_completeness_rows_and_text():
    P = matrix(SMALL)
    # t = 3: solid = 20 + 3 + 5 + 100 + 6 = 134
    assert diploid.completeness_rows(P, 3) == [("asm", 3, 134, 109, 113, 3), ("alt", 3, 134, 111, 116, 1), ("both", 3, 134, 114, 122, 3)]
    # a threshold of 0 counts as 1: column 0 is never solid
    assert diploid.completeness_rows(P, 0) == diploid.completeness_rows(P, 1)
    assert diploid.completeness_rows(P, 1)[0] == ("asm", 1, 146, 110, 113, 3)
    text = diploid.completeness_text(25, diploid.completeness_rows(P, 3))
    assert text == ("#set\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tdistinct\tnot_in_reads\n"
                    "asm\t25\t3\t134\t109\t81.3433\t113\t3\n"
                    "alt\t25\t3\t134\t111\t82.8358\t116\t1\n"
                    "both\t25\t3\t134\t114\t85.0746\t122\t3\n")
    rows = diploid.completeness_rows(matrix({(1, 0): 4, (3, 2): 9}), 5)            # no solid k-mer
    assert [r[2:] for r in rows] == [(0, 0, 13, 4), (0, 0, 9, 0), (0, 0, 13, 4)]
    assert diploid.completeness_text(31, rows).splitlines()[1] == "asm\t31\t5\t0\t0\tNA\t13\t4"
    assert diploid.completeness_log_text(rows) == "k-mer completeness: asm NA, alt NA, both NA (0 of 0 solid k-mers, threshold 5)"
    assert diploid.completeness_log_text(diploid.completeness_rows(P, 3)) == \
        "k-mer completeness: asm 81.3433 %, alt 82.8358 %, both 85.0746 % (114 of 134 solid k-mers, threshold 3)"


def test_the_asm_row_is_the_completeness_row_of_the_copy_number_spectrum():
    """rows 1 + 3 of P are the rows m >= 1 of spectrum(R, asm) added up: the asm row's five numbers are spectra.completeness_row's"""
    from jasper_amd import spectra
    P = matrix(SMALL)
    S = np.zeros((6, 10002), dtype=np.uint64)
    S[0] = P[0] + P[2]
    S[1] = P[1]
    S[4] = P[3]
    for t in (0, 1, 3, 31):
        assert diploid.completeness_rows(P, t)[0][1:] == spectra.completeness_row("asm", S, t)[1:]


K = 5
ASM_NAMES, ASM_LENGTHS = ["c1", "c2", "short"], [104, 24, 3]
# (windows, valid, unreliable, absent, private_solid, private_weak)
ASM_COUNTS = [(100, 100, 10, 4, 20, 7), (20, 20, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)]
ALT_NAMES, ALT_LENGTHS = ["h1", "gap"], [54, 12]
ALT_COUNTS = [(50, 48, 3, 0, 5, 3), (8, 0, 0, 0, 0, 0)]


def test_diploid_tsv_text():
    text = diploid.diploid_tsv_text(K, [("asm", ASM_NAMES, ASM_LENGTHS, ASM_COUNTS), ("alt", ALT_NAMES, ALT_LENGTHS, ALT_COUNTS)])
    lines = text.splitlines()
    assert lines[0].split("\t") == ["#set", "contig", "length", "windows", "valid", "unreliable", "absent", "QV_unreliable", "QV_absent", "private_solid",
                                    "private_weak", "shared_unreliable", "private_fraction"]
    assert [ln.split("\t")[:2] for ln in lines[1:]] == [["asm", "c1"], ["asm", "c2"], ["asm", "short"], ["asm", "*"], ["alt", "h1"], ["alt", "gap"], ["alt", "*"],
                                                        ["both", "*"]]
    q = report.qv_text
    assert lines[1] == "asm\tc1\t104\t100\t100\t10\t4\t%s\t%s\t20\t7\t3\t0.2700" % (q(10, 100, K), q(4, 100, K))
    assert lines[2] == "asm\tc2\t24\t20\t20\t0\t0\tinf\tinf\t0\t0\t0\t0.0000"
    assert lines[3] == "asm\tshort\t3\t0\t0\t0\t0\tNA\tNA\t0\t0\t0\tNA"                 # a contig without a valid window
    assert lines[4] == "asm\t*\t131\t120\t120\t10\t4\t%s\t%s\t20\t7\t3\t0.2250" % (q(10, 120, K), q(4, 120, K))
    assert lines[5] == "alt\th1\t54\t50\t48\t3\t0\t%s\tinf\t5\t3\t0\t0.1667" % q(3, 48, K)
    assert lines[6] == "alt\tgap\t12\t8\t0\t0\t0\tNA\tNA\t0\t0\t0\tNA"
    assert lines[7] == "alt\t*\t66\t58\t48\t3\t0\t%s\tinf\t5\t3\t0\t0.1667" % q(3, 48, K)
    assert lines[8] == "both\t*\t197\t178\t168\t13\t4\t%s\t%s\t25\t10\t3\t0.2083" % (q(13, 168, K), q(4, 168, K))
    assert q(10, 100, K) == "16.8086"                                                     # -10 log10(1 - 0.9^(1/5)), 0.9^0.2 = 0.9791484
    # the asm contigs' first columns are the rows of the k-mer report
    rep = report.qv_tsv_text(K, ASM_NAMES, [("asm", ASM_LENGTHS, [c[:4] for c in ASM_COUNTS])]).splitlines()[1:]
    for mine, theirs in zip(lines[1:5], rep):
        m, t = mine.split("\t"), theirs.split("\t")
        assert m[1] == t[0] and m[2:9] == t[2:9]
    empty = diploid.diploid_tsv_text(K, [("asm", [], [], []), ("alt", [], [], [])]).splitlines()
    assert empty[1:] == ["asm\t*\t0\t0\t0\t0\t0\tNA\tNA\t0\t0\t0\tNA", "alt\t*\t0\t0\t0\t0\t0\tNA\tNA\t0\t0\t0\tNA", "both\t*\t0\t0\t0\t0\t0\tNA\tNA\t0\t0\t0\tNA"]


def test_bed_text_lists_every_run():
    from jasper_amd.table import PAIRRUN_DTYPE
    runs = [(0, 10, 5, 1, 150), (0, 15, 1, 2, 0), (1, 0, 3, 2, 4), (0, 90, 2, 1, 2**40)]
    want = "c1\t10\t19\tsolid\t5\t30.00\nc1\t15\t20\tweak\t1\t0.00\nc2\t0\t7\tweak\t3\t1.33\nc1\t90\t96\tsolid\t2\t549755813888.00\n"
    assert diploid.bed_text(K, ASM_NAMES, runs) == want
    arr = np.array([(st, n, sr, seq, kind) for seq, st, n, kind, sr in runs], dtype=PAIRRUN_DTYPE)
    assert diploid.bed_text(K, ASM_NAMES, arr) == want
    assert diploid.bed_text(K, ASM_NAMES, []) == ""


def test_log_texts():
    assert diploid.qv_log_text(K, ASM_COUNTS, ALT_COUNTS) == "dense k-mer QV (unreliable k-mers): asm %s, alt %s, both %s" % (
        report.qv_text(10, 120, K), report.qv_text(3, 48, K), report.qv_text(13, 168, K))
    assert diploid.qv_log_text(K, [(5, 5, 0, 0, 0, 0)], [(0, 0, 0, 0, 0, 0)]) == "dense k-mer QV (unreliable k-mers): asm inf, alt NA, both inf"
    assert diploid.private_log_text(ASM_COUNTS, [1, 2, 3], ALT_COUNTS, [1]) == "private windows: asm 20 solid 7 weak in 3 runs; alt 5 solid 3 weak in 1 runs"


def test_files_are_written_through_a_tmp_name(tmp_path):
    p = tmp_path / "x.spectra_asm.tsv"
    diploid.write_atomic(str(p), diploid.spectra_asm_text(matrix(SMALL)))
    assert p.read_text() == diploid.spectra_asm_text(matrix(SMALL))
    assert [f.name for f in tmp_path.iterdir()] == ["x.spectra_asm.tsv"]
    assert diploid.write_atomic is report.write_atomic


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def test_kmerqc_parser_takes_alt(capsys):
    args = ["-a", "asm.fa", "-j", "db.jf", "--threshold", "4", "-o", "out/p"]
    without = kmerqc.parse_args(args)
    assert without["alt"] is None
    for argv in (["--alt", "h2.fa"] + args, args + ["--alt", "h2.fa"], args[:2] + ["--alt", "h2.fa"] + args[2:], args + ["--alt", "h2.fa", "--spectra", "--copies"]):
        got = kmerqc.parse_args(argv)
        assert got["alt"] == "h2.fa" and got["asm"] == "asm.fa"
    assert {k: v for k, v in kmerqc.parse_args(args + ["--alt", "h2.fa"]).items() if k != "alt"} == {k: v for k, v in without.items() if k != "alt"}
    with pytest.raises(SystemExit) as e:
        kmerqc.parse_args(args + ["--alt"])                                    # as the last argument: it takes a value, like -o
    assert e.value.code == 1 and capsys.readouterr().out == "Unknown option --alt\n"
    assert "--alt" in kmerqc.USAGE and "--alt" in kmerqc.__doc__
    assert "--alt" not in extensions.VALUE_FLAGS and "--alt" not in extensions.BOOL_FLAGS      # not one of the shared extension flags


def test_the_driver_rejects_alt(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["-a", "asm.fa", "--alt", "h2.fa"])
    assert e.value.code == 1 and capsys.readouterr().out == "Unknown option --alt\n"
    assert "--alt" not in cli.USAGE


def write_inputs(d):
    (d / "asm.fa").write_text(">c1 first\nACGTTGCAACGGTCAGTCCATGAC\nGGATC\n>c2\nTTGACCAGTNACCGGTTAAC\n")
    (d / "alt.fa").write_text(">h1\nACGTTGCAACGGTCAGACCATGACGGATC\n")
    (d / "reads.fq").write_text("@r\nACGTTGCAACGGTCAGTCCATGACGGATC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")


@pytest.mark.parametrize("alt,word", [("nowhere.fa", "does not exist"), ("empty.fa", "does not exist or is empty"), ("asm.fa", "itself"), ("link.fa", "itself")])
def test_a_bad_alt_file_ends_the_run_before_anything_is_counted(tmp_path, monkeypatch, capsys, alt, word):
    write_inputs(tmp_path)
    (tmp_path / "empty.fa").write_text("")
    os.symlink(str(tmp_path / "asm.fa"), str(tmp_path / "link.fa"))              # the same file under another name
    monkeypatch.chdir(tmp_path)

    def no_table(*a, **k):
        raise AssertionError("a table was made")
    monkeypatch.setattr(kmerqc, "KmerTable", no_table)
    with pytest.raises(SystemExit) as e:
        kmerqc.run(["-a", "asm.fa", "--alt", alt, "-r", "reads.fq", "-k", "5", "--threshold", "1"])
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert "--alt" in err and word in err
    assert sorted(f.name for f in tmp_path.iterdir()) == ["alt.fa", "asm.fa", "empty.fa", "link.fa", "reads.fq"]


class FakeTable:
    """records what is counted into it and what is asked of it; the results are zeros of the right shape"""
    made = []

    def __init__(self, k, min_slots=0, device=0):
        self.k, self.device, self.calls, self.closed = int(k), device, [], False
        FakeTable.made.append(self)

    def count_files(self, files):
        self.calls.append(("count_files", tuple(files)))

    def count_bases(self, text):
        self.calls.append(("count_bases", text))

    def histo_rows(self):
        return [(1, 50), (2, 10), (20, 300), (21, 200)]

    def _counts(self, seqs, width):
        return [(max(0, len(s) - self.k + 1),) * 2 + (0,) * (width - 2) for s in seqs]

    def kmer_report(self, seqs, thre):
        from jasper_amd.table import KMERRUN_DTYPE, KmerReport
        return KmerReport(self._counts(seqs, 4), np.zeros(0, dtype=KMERRUN_DTYPE), 0.0, False)

    def spectrum(self, asm):
        from jasper_amd.table import KmerSpectrum
        self.calls.append(("spectrum", asm))
        return KmerSpectrum(np.zeros((6, 10002), dtype=np.uint64), 0.0)

    def copy_report(self, asm, seqs, thre, peak):
        from jasper_amd.table import COPYRUN_DTYPE, CopyReport
        self.calls.append(("copy_report", asm))
        return CopyReport(self._counts(seqs, 6), np.zeros(0, dtype=COPYRUN_DTYPE), 0.0, False)

    def spectrum_pair(self, asm, alt):
        from jasper_amd.table import PairSpectrum
        assert not asm.closed and not alt.closed
        self.calls.append(("spectrum_pair", asm, alt))
        return PairSpectrum(matrix(SMALL), 0.0)

    def pair_scan(self, other, seqs, thre):
        from jasper_amd.table import PAIRRUN_DTYPE, PairScan
        assert not other.closed
        self.calls.append(("pair_scan", other, tuple(seqs), thre))
        return PairScan(self._counts(seqs, 6), np.zeros(0, dtype=PAIRRUN_DTYPE), 0.0, False)

    def close(self):
        self.closed = True


ASM_TEXT = "ACGTTGCAACGGTCAGTCCATGACGGATC" + "N" + "TTGACCAGTNACCGGTTAAC"
ALT_TEXT = "ACGTTGCAACGGTCAGACCATGACGGATC"


def run_with_fake(tmp_path, monkeypatch, flags):
    from jasper_amd import table as table_mod
    write_inputs(tmp_path)
    monkeypatch.chdir(tmp_path)
    FakeTable.made = []
    monkeypatch.setattr(kmerqc, "KmerTable", FakeTable)
    monkeypatch.setattr(table_mod, "KmerTable", FakeTable)            # (extensions.assembly_table looks it up there)
    assert kmerqc.run(["-a", "asm.fa", "-r", "reads.fq", "-k", "5", "--threshold", "2", "-o", "p"] + flags) == 0
    reads = FakeTable.made[0]
    assert reads.calls[0] == ("count_files", ("reads.fq",)) and all(t.closed for t in FakeTable.made)
    counted = [t for t in FakeTable.made[1:] for c in t.calls if c[0] == "count_bases"]
    return reads, counted, sorted(f.name for f in tmp_path.iterdir() if f.name.startswith("p."))


NEW_FILES = ["p.diploid.completeness.tsv", "p.diploid.tsv", "p.private.alt.bed", "p.private.asm.bed", "p.spectra_asm.tsv"]


def test_alt_alone_counts_each_haplotype_once_and_makes_no_copy_number_spectrum(tmp_path, monkeypatch, capsys):
    reads, counted, files = run_with_fake(tmp_path, monkeypatch, ["--alt", "alt.fa"])
    assert [t.calls for t in counted] == [[("count_bases", ASM_TEXT)], [("count_bases", ALT_TEXT)]]
    a1, a2 = counted
    kinds = [c[0] for c in reads.calls]
    assert "spectrum" not in kinds and "copy_report" not in kinds
    assert reads.calls[1:] == [("spectrum_pair", a1, a2), ("pair_scan", a2, tuple(ASM_TEXT.replace("NTTG", " TTG").split()), 2), ("pair_scan", a1, (ALT_TEXT,), 2)]
    assert files == sorted(NEW_FILES + ["p.kmer_qv.tsv", "p.unreliable.bed"])
    assert (tmp_path / "p.spectra_asm.tsv").read_text() == diploid.spectra_asm_text(matrix(SMALL))
    assert (tmp_path / "p.diploid.completeness.tsv").read_text() == diploid.completeness_text(5, diploid.completeness_rows(matrix(SMALL), 2))
    rows = [ln.split("\t")[:3] for ln in (tmp_path / "p.diploid.tsv").read_text().splitlines()[1:]]
    assert rows == [["asm", "c1", "29"], ["asm", "c2", "20"], ["asm", "*", "49"], ["alt", "h1", "29"], ["alt", "*", "29"], ["both", "*", "78"]]
    out = capsys.readouterr().out
    assert "Diploid k-mer completeness: asm" in out and "Diploid dense k-mer QV (unreliable k-mers): asm inf, alt inf, both inf" in out
    assert "Diploid private windows: asm 0 solid 0 weak in 0 runs; alt 0 solid 0 weak in 0 runs in p.private.asm.bed and p.private.alt.bed" in out


def test_the_asm_table_is_counted_once_for_alt_spectra_and_copies(tmp_path, monkeypatch, capsys):
    reads, counted, files = run_with_fake(tmp_path, monkeypatch, ["--alt", "alt.fa", "--spectra", "--copies", "--peak", "20"])
    assert [t.calls for t in counted] == [[("count_bases", ASM_TEXT)], [("count_bases", ALT_TEXT)]], "A1 is counted once, A2 once"
    a1, a2 = counted
    assert [c[:2] for c in reads.calls[1:4]] == [("spectrum", a1), ("copy_report", a1), ("spectrum_pair", a1)]
    assert set(NEW_FILES) < set(files) and {"p.spectra_cn.tsv", "p.completeness.tsv", "p.copies.tsv", "p.copies.bed"} < set(files)
    with_alt = {f: (tmp_path / f).read_bytes() for f in files if f not in NEW_FILES}
    log_with = [ln.split("] ", 1)[1] for ln in capsys.readouterr().out.splitlines()]
    for f in files:
        os.remove(str(tmp_path / f))
    # without --alt: the other files are byte for byte the same, the log lines are the same up to the three new ones, one table fewer
    _, counted, files = run_with_fake(tmp_path, monkeypatch, ["--spectra", "--copies", "--peak", "20"])
    assert [t.calls for t in counted] == [[("count_bases", ASM_TEXT)]]
    assert {f: (tmp_path / f).read_bytes() for f in files} == with_alt
    log_without = [ln.split("] ", 1)[1] for ln in capsys.readouterr().out.splitlines()]
    assert log_with[:len(log_without)] == log_without and len(log_with) == len(log_without) + 3
    assert all(ln.startswith("Diploid ") for ln in log_with[len(log_without):])


def test_timing_line(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("JASPER_AMD_TIMING", "1")
    run_with_fake(tmp_path, monkeypatch, ["--alt", "alt.fa"])
    assert "[diploid] device seconds: join 0.000000 scan asm 0.000000 scan alt 0.000000" in capsys.readouterr().err
