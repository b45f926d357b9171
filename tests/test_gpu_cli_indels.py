"""GPU: `python -m jasper_amd.cli ... --indels` and `python -m jasper_amd.kmerqc ... --indels` on the files of the golden case gaps_k25
(one 6006-base contig with length errors of several sizes, its reads).

Without the flag nothing changes; with it the three new files equal what this file computes with the restatement of
tests/test_indels_host.py over a Python dict of the reads' k-mers, on asm.fa and on the polished FASTA it reads back, and with its own
left alignment; with --variants as well the variant files are those of --variants alone."""
import gzip
import os
import re
import shutil

import pytest

from golden_util import Case
from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_cli_variants import VARIANT_FILES
from test_gpu_copies import dict_counter, kmer_dict
from test_indels_host import restate

pytestmark = pytest.mark.gpu
CASE = "gaps_k25"
K = 25
MAX_LEN = 4
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
INDEL_FILES = ("asm.fa.indels.after.vcf", "asm.fa.indels.before.vcf", "asm.fa.indels.tsv")
COMMON = ("asm.fa.polished.fasta", "asm.fa.fixes.csv", "jfhisto%d.csv" % K, "threshold.txt")
TSV_HEADER = "#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error"
BASES = "ACGTacgt"


def write_inputs(d):
    c = Case(CASE)
    assert c.k == K
    shutil.copy(os.path.join(c.dir, "batch.fa"), d / "asm.fa")
    with open(d / "reads.fq", "wb") as f:
        f.write(gzip.open(os.path.join(c.dir, "reads.fq.gz")).read())
    with open(d / "threshold.txt", "w") as f:
        f.write("%d\n" % c.thre)


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("variants", ["--variants"]), ("indels", ["--indels"]), ("both", ["--variants", "--indels", "--indel-max-len", str(MAX_LEN)])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d1 = runs["indels"][0]
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    rd = kmer_dict(open(d1 / "reads.fq", "rb").read().split(b"\n")[1::4], K)
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert pnames == names and thre >= 1
    count = dict_counter(rd)
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, before=restate(seqs, K, count, thre, MAX_LEN), after=restate(pseqs, K, count, thre, MAX_LEN))


def check_tsv(text, names, stages):
    lines = text.splitlines()
    want = []
    for i, n in enumerate(names):
        for stage, seqs, counts in stages:
            want.append((n, stage, len(seqs[i])) + tuple(counts[i]))
    for stage, seqs, counts in stages:
        want.append(("*", stage, sum(len(s) for s in seqs)) + tuple(sum(c[j] for c in counts) for j in range(4)))
    assert lines[0] == TSV_HEADER and text.endswith("\n")
    assert lines[1:] == ["\t".join(str(v) for v in w) for w in want]


def vcf_line(names, seqs, rec):
    """(sort key, line) of one record of the restatement: the rules of the README restated -- a deletion at q moves to q - 1 while
    q > 1, s[q-1] is a base and folds to what s[q+L-1] folds to; an insertion of x^L moves while q > 1 and s[q-1] folds to x; POS = q"""
    seq, q, typ, L, x, rmin, amin, kind = rec
    s = seqs[seq]
    if typ == "del":
        while q > 1 and s[q - 1] in BASES and s[q - 1].upper() == s[q + L - 1].upper():
            q -= 1
        ref, alt = s[q - 1:q + L].upper(), s[q - 1].upper()
    else:
        while q > 1 and s[q - 1].upper() == x:
            q -= 1
        ref, alt = s[q - 1].upper(), s[q - 1].upper() + x * L
    line = "%s\t%d\t.\t%s\t%s\t.\t.\tKIND=%s;TYPE=%s;LEN=%d;RC=%d;AC=%d" % (names[seq], q, ref, alt, {1: "het", 2: "error"}[kind], typ, L, rmin, amin)
    return (seq, q, {"ins": 1, "del": 2}[typ], L, alt), line


def check_vcf(text, names, seqs, recs):
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == "##fileformat=VCFv4.2" and "max_len=%d" % MAX_LEN in lines[1]
    assert [ln for ln in lines if ln.startswith("##contig")] == ["##contig=<ID=%s,length=%d>" % (n, len(s)) for n, s in zip(names, seqs)]
    assert [re.match(r"##INFO=<ID=(\w+),", ln).group(1) for ln in lines if ln.startswith("##INFO")] == ["KIND", "TYPE", "LEN", "RC", "AC"]
    head = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    assert all(ln.startswith("##") for ln in lines[:head])
    assert lines[head + 1:] == [ln for _, ln in sorted(vcf_line(names, seqs, r) for r in recs)]
    for ln in lines[head + 1:]:                                          # REF starts at the sequence's own bytes at POS (1-based)
        f = ln.split("\t")
        assert seqs[names.index(f[0])][int(f[1]) - 1:int(f[1]) - 1 + len(f[3])].upper() == f[3] and f[4][0] == f[3][0]


def log_line(c0, c1):
    return "Indel scan: before polishing %d het and %d error insertions, %d het and %d error deletions; after polishing %d het and %d error insertions, " \
           "%d het and %d error deletions" % tuple(sum(c[j] for c in cs) for cs in (c0, c1) for j in range(4))


def test_one_gpu_indel_files_and_nothing_else_changes(runs, truth):
    (d0, p0), (d1, p1) = runs["plain"], runs["indels"]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    for fn in COMMON:
        assert os.path.isfile(d0 / fn), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "Indel scan" in m]
    assert len(extra) == 1 and [m for m in m1 if m not in extra] == m0    # same log lines otherwise ...
    assert "After Polishing: Q value" in m1[m1.index(extra[0]) - 1]          # ... the new one right after the reference's two Q lines
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(INDEL_FILES)      # a run without --indels writes today's file set
    assert set(os.listdir(d0)) <= set(os.listdir(d1))
    t = truth
    (c0, r0), (c1, r1) = t["before"], t["after"]
    check_tsv(open(d1 / "asm.fa.indels.tsv").read(), t["names"], [("before", t["seqs"], c0), ("after", t["pseqs"], c1)])
    check_vcf(open(d1 / "asm.fa.indels.before.vcf").read(), t["names"], t["seqs"], r0)
    check_vcf(open(d1 / "asm.fa.indels.after.vcf").read(), t["names"], t["pseqs"], r1)
    assert extra[0] == log_line(c0, c1)
    # the case holds what the scan is for: insertions and deletions before polishing, fewer after it
    assert {r[2] for r in r0} == {"ins", "del"} and len(r1) < len(r0)


def test_variants_and_indels_together_write_the_variant_files_of_variants_alone(runs):
    (d0, _), (dv, pv), (di, _), (db, pb) = runs["plain"], runs["variants"], runs["indels"], runs["both"]
    assert sorted(set(os.listdir(db)) - set(os.listdir(d0))) == sorted(VARIANT_FILES + INDEL_FILES)
    assert sorted(set(os.listdir(dv)) - set(os.listdir(d0))) == sorted(VARIANT_FILES)
    for fn in COMMON + VARIANT_FILES:
        assert open(db / fn, "rb").read() == open(dv / fn, "rb").read(), fn
    for fn in INDEL_FILES:
        assert open(db / fn, "rb").read() == open(di / fn, "rb").read(), fn
    mv, mb = messages(pv.stdout), messages(pb.stdout)
    extra = [m for m in mb if "Indel scan" in m]
    assert len(extra) == 1 and [m for m in mb if m not in extra] == mv
    assert "Variant scan" in mb[mb.index(extra[0]) - 1]                     # the new line comes after the existing ones
    assert not [fn for fn in os.listdir(db) if fn.endswith(".tmp")]


def test_kmerqc_indels_reproduces_the_before_rows(runs, truth, tmp_path):
    import subprocess
    import sys
    from test_gpu_cli_spectra import ROOT
    d1 = runs["both"][0]
    seen = set(os.listdir(d1))
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(truth["thre"])]
    p = cli(d1, base + ["-o", str(tmp_path / "qc"), "--indels", "--variants"], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == ["qc.indels.tsv", "qc.indels.vcf", "qc.kmer_qv.tsv", "qc.unreliable.bed", "qc.variants.tsv", "qc.variants.vcf"]
    driver = open(d1 / "asm.fa.indels.tsv").read().splitlines()
    want = [driver[0]] + [ln.replace("\tbefore\t", "\tasm\t", 1) for ln in driver[1:] if "\tbefore\t" in ln]
    assert len(want) == 3 and open(tmp_path / "qc.indels.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.indels.vcf").read() == open(d1 / "asm.fa.indels.before.vcf").read()
    assert open(tmp_path / "qc.variants.vcf").read() == open(d1 / "asm.fa.variants.before.vcf").read()
    c0 = truth["before"][0]
    assert [m for m in messages(p.stdout) if "Indel scan" in m] == ["Indel scan: %d het and %d error insertions, %d het and %d error deletions in %s.indels.vcf" % (
        tuple(sum(c[j] for c in c0) for j in range(4)) + (tmp_path / "qc",))]
    # without the flag kmerqc writes what it wrote before
    cli(d1, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("q0.")) == ["q0.kmer_qv.tsv", "q0.unreliable.bed"]
    # a threshold of 0, or a length outside 1..16: exit status 1 and a message, no file
    for flags, word in ((["--threshold", "0", "--indels"], "--indels"), (["--threshold", "3", "--indels", "--indel-max-len", "17"], "--indel-max-len")):
        p = subprocess.run([sys.executable, "-m", "jasper_amd.kmerqc"] + base[:4] + flags + ["-o", str(tmp_path / "qz")], cwd=d1,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1 and word in p.stderr and not [fn for fn in os.listdir(tmp_path) if fn.startswith("qz.")]
