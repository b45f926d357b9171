"""GPU: `python -m jasper_amd.cli ... --variants` and `python -m jasper_amd.kmerqc ... --variants` on the files of the golden case
diploid_k25 (one 4999-base contig of a diploid genome, ten heterozygous sites, its reads).

Without the flag nothing changes; with it the three new files equal what this file computes with the restatement of
tests/test_gpu_variants.py over a Python dict of the reads' k-mers, on asm.fa and on the polished FASTA it reads back."""
import gzip
import os
import re
import shutil

import pytest

from golden_util import Case
from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_copies import dict_counter, kmer_dict
from test_gpu_variants import ERROR, HET, restate

pytestmark = pytest.mark.gpu
CASE = "diploid_k25"
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
VARIANT_FILES = ("asm.fa.variants.after.vcf", "asm.fa.variants.before.vcf", "asm.fa.variants.tsv")
COMMON = ("asm.fa.polished.fasta", "asm.fa.fixes.csv", "jfhisto%d.csv" % K, "threshold.txt")
TSV_HEADER = "#contig\tstage\tlength\tevaluated\thet\terror\thet_per_kb"
PEAK = 18      # (the run with every extension: --copies wants a single-copy read count; any will do here)


def write_inputs(d):
    """the case's batch.fa as the assembly, its reads, and its threshold: the histogram of so small a read set has no local minimum
    (src/jellyfish.py exits 1 on it, meta.json), and the driver, as src/jasper.sh:195-206, then uses the threshold.txt it finds"""
    c = Case(CASE)
    assert c.k == K
    shutil.copy(os.path.join(c.dir, "batch.fa"), d / "asm.fa")
    with open(d / "reads.fq", "wb") as f:
        f.write(gzip.open(os.path.join(c.dir, "reads.fq.gz")).read())
    with open(d / "threshold.txt", "w") as f:
        f.write("%d\n" % c.thre)
    return c.thre


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("variants", ["--variants"]), ("all", ["--variants", "--copies", "--peak", str(PEAK), "--spectra", "--report"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d1 = runs["variants"][0]
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    rd = kmer_dict(open(d1 / "reads.fq", "rb").read().split(b"\n")[1::4], K)
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["dip:0"] and pnames == names and thre == Case(CASE).thre
    count = dict_counter(rd)
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, before=restate(seqs, K, count, thre), after=restate(pseqs, K, count, thre))


def check_tsv(text, names, stages):
    """stages: [(stage, sequences, counts)]; integers exactly, het_per_kb to 1e-4 (printed to four decimals)"""
    lines = text.splitlines()
    want = []
    for i, n in enumerate(names):
        for stage, seqs, counts in stages:
            want.append((n, stage, len(seqs[i])) + tuple(counts[i]))
    for stage, seqs, counts in stages:
        want.append(("*", stage, sum(len(s) for s in seqs)) + tuple(sum(c[j] for c in counts) for j in range(3)))
    assert lines[0] == TSV_HEADER and text.endswith("\n") and len(lines) == 1 + len(want)
    for ln, w in zip(lines[1:], want):
        f = ln.split("\t")
        assert f[:6] == [str(v) for v in w], ln
        if w[3] == 0:
            assert f[6] == "NA", ln
        else:
            assert re.match(r"^\d+\.\d{4}$", f[6]) and abs(float(f[6]) - 1000.0 * w[4] / w[3]) <= 1e-4, ln


def check_vcf(text, names, seqs, recs):
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == "##fileformat=VCFv4.2"
    assert [ln for ln in lines if ln.startswith("##contig")] == ["##contig=<ID=%s,length=%d>" % (n, len(s)) for n, s in zip(names, seqs)]
    assert [re.match(r"##INFO=<ID=(\w+),", ln).group(1) for ln in lines if ln.startswith("##INFO")] == ["KIND", "RC", "AC"]
    head = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    assert all(ln.startswith("##") for ln in lines[:head])
    want = ["%s\t%d\t.\t%s\t%s\t.\t.\tKIND=%s;RC=%d;AC=%d" % (names[seq], pos + 1, ref, alt, {HET: "het", ERROR: "error"}[kind], rmin, amin)
            for seq, pos, ref, alt, rmin, amin, kind in recs]
    assert lines[head + 1:] == want
    for ln in want:                                                      # REF is the sequence's own base at POS (1-based)
        f = ln.split("\t")
        assert seqs[names.index(f[0])][int(f[1]) - 1].upper() == f[3]


def log_line(c0, c1):
    return "Variant scan: before polishing %d het and %d error sites; after polishing %d het and %d error sites" % (
        sum(c[1] for c in c0), sum(c[2] for c in c0), sum(c[1] for c in c1), sum(c[2] for c in c1))


def test_one_gpu_variant_files_and_nothing_else_changes(runs, truth):
    (d0, p0), (d1, p1) = runs["plain"], runs["variants"]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    for fn in COMMON:
        assert os.path.isfile(d0 / fn), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "Variant scan" in m]
    assert len(extra) == 1 and [m for m in m1 if m not in extra] == m0    # same log lines otherwise ...
    assert "After Polishing: Q value" in m1[m1.index(extra[0]) - 1]          # ... the new one right after the reference's two Q lines
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(VARIANT_FILES)
    assert set(os.listdir(d0)) <= set(os.listdir(d1))
    t = truth
    (c0, r0, _), (c1, r1, _) = t["before"], t["after"]
    check_tsv(open(d1 / "asm.fa.variants.tsv").read(), t["names"], [("before", t["seqs"], c0), ("after", t["pseqs"], c1)])
    check_vcf(open(d1 / "asm.fa.variants.before.vcf").read(), t["names"], t["seqs"], r0)
    check_vcf(open(d1 / "asm.fa.variants.after.vcf").read(), t["names"], t["pseqs"], r1)
    assert extra[0] == log_line(c0, c1)
    # the case holds what the scan is for: its ten heterozygous sites, before and after (the polisher must not touch a solid allele),
    # and polishing does not add error sites
    assert (c0[0][1], c0[0][2]) == (10, 0) and c1[0][1] >= 10
    assert sum(c[2] for c in c1) <= sum(c[2] for c in c0)


def test_variants_with_every_other_extension_gives_the_union(runs):
    from test_gpu_cli_copies import COPIES_FILES
    from test_gpu_cli_spectra import REPORT_FILES, SPECTRA_FILES
    (d0, _), (d1, _), (d2, p2) = runs["plain"], runs["variants"], runs["all"]
    assert sorted(set(os.listdir(d2)) - set(os.listdir(d0))) == sorted(VARIANT_FILES + COPIES_FILES + SPECTRA_FILES + REPORT_FILES)
    for fn in COMMON + VARIANT_FILES:
        assert open(d2 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    m2 = messages(p2.stdout)
    assert [sum(what in m for m in m2) for what in ("dense k-mer QV", "k-mer completeness", "Copy-number scan", "Variant scan")] == [2, 2, 2, 1]
    ix = [min(i for i, m in enumerate(m2) if what in m) for what in ("dense k-mer QV", "k-mer completeness", "Copy-number scan", "Variant scan", "Polished sequence is in")]
    assert ix == sorted(ix)                                                # the new line comes after the existing ones
    assert not [fn for fn in os.listdir(d2) if fn.endswith(".tmp")]


def test_kmerqc_variants_reproduces_the_before_rows(runs, truth, tmp_path):
    import subprocess
    import sys
    from test_gpu_cli_spectra import ROOT
    d1 = runs["variants"][0]
    seen = set(os.listdir(d1))
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(truth["thre"])]
    p = cli(d1, base + ["-o", str(tmp_path / "qc"), "--variants"], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == ["qc.kmer_qv.tsv", "qc.unreliable.bed", "qc.variants.tsv", "qc.variants.vcf"]
    driver = open(d1 / "asm.fa.variants.tsv").read().splitlines()
    want = [driver[0]] + [ln.replace("\tbefore\t", "\tasm\t", 1) for ln in driver[1:] if "\tbefore\t" in ln]
    assert len(want) == 3 and open(tmp_path / "qc.variants.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.variants.vcf").read() == open(d1 / "asm.fa.variants.before.vcf").read()
    c0 = truth["before"][0]
    assert [m for m in messages(p.stdout) if "Variant scan" in m] == ["Variant scan: %d het and %d error sites in %s.variants.vcf" % (
        sum(c[1] for c in c0), sum(c[2] for c in c0), tmp_path / "qc")]
    # without the flag kmerqc writes what it wrote before
    cli(d1, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("q0.")) == ["q0.kmer_qv.tsv", "q0.unreliable.bed"]
    assert open(tmp_path / "q0.kmer_qv.tsv").read() == open(tmp_path / "qc.kmer_qv.tsv").read()
    # --threshold 0 with --variants: exit status 1 and a message, no file
    p = subprocess.run([sys.executable, "-m", "jasper_amd.kmerqc"] + base[:4] + ["--threshold", "0", "-o", str(tmp_path / "qz"), "--variants"], cwd=d1,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "--variants" in p.stderr and not [fn for fn in os.listdir(tmp_path) if fn.startswith("qz.")]
