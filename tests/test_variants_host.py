"""CPU: jasper_amd/variants.py -- the texts of `*.variants.tsv` / `*.variants*.vcf` and the log line for hand-made counters and
records -- and the parsers' new flag.  The expected texts are written out here by hand from the formats in README.md."""
import numpy as np
import pytest

from jasper_amd import cli, kmerqc, report, variants
from jasper_amd.table import VARIANT_DTYPE

NAMES = ["ctg1", "ctg2", "ctg3"]
# (evaluated, het, error)
BEFORE = [(2000, 5, 2), (500, 0, 1), (0, 0, 0)]
AFTER = [(2001, 5, 0), None, (40, 1, 0)]
# (seq, pos, ref, alt, ref_min, alt_min, kind), not in order
RECS = [(1, 7, "G", "A", 0, 21, 2), (0, 99, "A", "T", 12, 9, 1), (0, 99, "A", "C", 12, 5, 1), (0, 0, "c".upper(), "G", 2, 30, 2), (2, 1999, "T", "C", 4294967295, 8, 1)]


def test_tsv_text():
    text = variants.variants_tsv_text(NAMES, [("before", [2048, 548, 30], BEFORE), ("after", [2049, 0, 88], AFTER)])
    want = ("#contig\tstage\tlength\tevaluated\thet\terror\thet_per_kb\n"
            "ctg1\tbefore\t2048\t2000\t5\t2\t2.5000\n"
            "ctg1\tafter\t2049\t2001\t5\t0\t2.4988\n"
            "ctg2\tbefore\t548\t500\t0\t1\t0.0000\n"
            "ctg2\tafter\t0\t0\t0\t0\tNA\n"                                   # a contig the polished FASTA lacks
            "ctg3\tbefore\t30\t0\t0\t0\tNA\n"                                 # too short: nothing evaluated
            "ctg3\tafter\t88\t40\t1\t0\t25.0000\n"
            "*\tbefore\t2626\t2500\t5\t3\t2.0000\n"
            "*\tafter\t2137\t2041\t6\t0\t2.9397\n")
    assert text == want
    one = variants.variants_tsv_text(["a"], [("asm", [40], [(10, 1, 2)])])
    assert one.splitlines()[1:] == ["a\tasm\t40\t10\t1\t2\t100.0000", "*\tasm\t40\t10\t1\t2\t100.0000"]
    assert variants.totals(AFTER) == (2041, 6, 0)
    assert variants.het_per_kb_text(0, 0) == "NA" and variants.het_per_kb_text(1, 3) == "333.3333"


def test_vcf_text_is_one_based_and_ordered():
    text = variants.vcf_text(25, 4, NAMES, [2048, 548, 2030], RECS)
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == "##fileformat=VCFv4.2"
    assert [ln for ln in lines if ln.startswith("##contig")] == ["##contig=<ID=ctg1,length=2048>", "##contig=<ID=ctg2,length=548>", "##contig=<ID=ctg3,length=2030>"]
    assert [ln.split(",")[0] for ln in lines if ln.startswith("##INFO")] == ["##INFO=<ID=KIND", "##INFO=<ID=RC", "##INFO=<ID=AC"]
    head = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    assert all(ln.startswith("##") for ln in lines[:head])
    assert lines[head + 1:] == ["ctg1\t1\t.\tC\tG\t.\t.\tKIND=error;RC=2;AC=30",                  # pos 0 is POS 1
                                "ctg1\t100\t.\tA\tC\t.\t.\tKIND=het;RC=12;AC=5",                  # two alternatives of one position: A < C < G < T
                                "ctg1\t100\t.\tA\tT\t.\t.\tKIND=het;RC=12;AC=9",
                                "ctg2\t8\t.\tG\tA\t.\t.\tKIND=error;RC=0;AC=21",
                                "ctg3\t2000\t.\tT\tC\t.\t.\tKIND=het;RC=4294967295;AC=8"]
    # the same from the structured array KmerTable.variant_scan returns (letters as byte values)
    arr = np.array([(pos, seq, rmin, amin, ord(ref), ord(alt), kind, 0) for seq, pos, ref, alt, rmin, amin, kind in sorted(RECS)], dtype=VARIANT_DTYPE)
    assert arr.itemsize == 24 and variants.vcf_text(25, 4, NAMES, [2048, 548, 2030], arr) == text
    none = variants.vcf_text(25, 4, ["a"], [10], [])
    assert none.splitlines()[-1].startswith("#CHROM") and "##contig=<ID=a,length=10>" in none


def test_a_contig_missing_after_polishing_and_the_log_line():
    names1 = ["ctg3", "ctg1"]
    len1, cnt1 = [88, 2049], [AFTER[2], AFTER[0]]
    len1a, cnt1a = variants.align(NAMES, names1, len1, cnt1)
    assert (len1a, cnt1a) == ([2049, 0, 88], AFTER) and variants.align is report.align
    assert "ctg2\tafter\t0\t0\t0\t0\tNA\n" in variants.variants_tsv_text(NAMES, [("before", [2048, 548, 30], BEFORE), ("after", len1a, cnt1a)])
    assert variants.log_text(BEFORE, cnt1a) == "Variant scan: before polishing 5 het and 3 error sites; after polishing 6 het and 0 error sites"
    assert variants.stage_log_text([(1, 0, 0)]) == "0 het and 0 error sites"
    # the `after` VCF is in the polished FASTA's own order and coordinates
    text = variants.vcf_text(25, 4, names1, len1, [(0, 4, "A", "C", 9, 9, 1), (1, 0, "T", "G", 0, 7, 2)])
    assert text.splitlines()[-2:] == ["ctg3\t5\t.\tA\tC\t.\t.\tKIND=het;RC=9;AC=9", "ctg1\t1\t.\tT\tG\t.\t.\tKIND=error;RC=0;AC=7"]


def test_files_are_written_through_a_tmp_name(tmp_path):
    p = tmp_path / "x.variants.vcf"
    variants.write_atomic(str(p), variants.vcf_text(25, 4, NAMES, [1, 2, 3], RECS))
    assert p.read_text() == variants.vcf_text(25, 4, NAMES, [1, 2, 3], RECS)
    assert [f.name for f in tmp_path.iterdir()] == ["x.variants.vcf"]
    assert variants.write_atomic is report.write_atomic


def test_cli_parser_takes_the_flag(capsys):
    without = cli.parse_args(["-a", "x/asm.fa", "-k", "25"])
    assert without.variants is False
    o = cli.parse_args(["-a", "x/asm.fa", "--variants", "-k", "25"])
    assert o.variants is True
    a, b = dict(vars(o)), dict(vars(without))
    del a["variants"], b["variants"]
    assert a == b and b["kmer"] == "25" and b["spectra"] is False and b["report"] is False and b["copies"] is False
    every = cli.parse_args(["--variants", "--copies", "--spectra", "--report"])
    assert every.variants and every.copies and every.spectra and every.report
    with pytest.raises(SystemExit):
        cli.parse_args(["--variant"])
    with pytest.raises(SystemExit) as e:
        cli.scan_variants(None, [], 0)                        # a threshold of 0 ends the run before anything is scanned
    assert e.value.code == 1 and "--variants" in capsys.readouterr().err


def test_kmerqc_parser_takes_the_flag(tmp_path, capsys):
    args = ["-a", "asm.fa", "-j", "db.jf", "--threshold", "4", "-o", "out/p"]
    without = kmerqc.parse_args(args)
    assert without["variants"] is False
    got = kmerqc.parse_args(["--variants"] + args)
    assert got["variants"] is True and {k: v for k, v in got.items() if k != "variants"} == {k: v for k, v in without.items() if k != "variants"}
    both = kmerqc.parse_args(args + ["--copies", "--variants", "--spectra"])
    assert both["variants"] and both["copies"] and both["spectra"]
    assert "--variants" in kmerqc.USAGE
    # --threshold 0 with --variants: exit status 1 and a message, before any table is made
    asm = tmp_path / "asm.fa"
    asm.write_text(">a\nACGT\n")
    with pytest.raises(SystemExit) as e:
        kmerqc.run(["-a", str(asm), "-j", "nosuch.jf", "--threshold", "0", "--variants"])
    assert e.value.code == 1 and "--variants" in capsys.readouterr().err
