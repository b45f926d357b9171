"""GPU: `python -m jasper_amd.cli ... --spectra` and `python -m jasper_amd.kmerqc ... --spectra` on a small synthetic case.

Without the flag nothing changes; with it the three new files equal what this file computes with Python dicts from reads.fq,
asm.fa and the polished FASTA it reads back (its own restatement of the semantics in include/jasper_hip.h and of the file
formats in README.md)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
SPECTRA_FILES = ("asm.fa.completeness.tsv", "asm.fa.spectra_cn.after.tsv", "asm.fa.spectra_cn.before.tsv")
REPORT_FILES = ("asm.fa.kmer_qv.tsv", "asm.fa.unreliable.after.bed", "asm.fa.unreliable.before.bed")
COMMON = ("asm.fa.polished.fasta", "asm.fa.fixes.csv", "jfhisto%d.csv" % K, "threshold.txt")
LABELS = ("0", "1", "2", "3", "4", ">4")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def write_inputs(d):
    """three contigs; the second has a stretch in lower case, the third holds a piece of the first once more and a piece of the
    second twice more (rows 2 and 3 of the spectrum)"""
    from jasper_amd import synth
    rng = np.random.default_rng(31)
    genome = synth.make_genome(rng, 45_000)
    reads = synth.make_reads_stream(rng, genome, 60, 150, 0.003).reshape(-1, 151)[:, :150]
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + b"I" * 150 + b"\n")
    asm = synth.make_assembly(rng, genome, err=3e-3, n_every=17_000, n_len=30).tobytes()
    cuts = [0, 21_000, 33_500, len(asm)]
    with open(d / "asm.fa", "wb") as f:
        for i in range(3):
            s = asm[cuts[i]:cuts[i + 1]]
            if i == 1:
                s = s[:400] + s[400:900].lower() + s[900:]
            if i == 2:
                s = s + b"NNNNNNNNNN" + asm[2000:3500] + b"NNNNNNNNNN" + asm[25_000:26_000] + b"NNNNNNNNNN" + asm[25_000:26_000]
            f.write(b">ctg%d sample=%d\n" % (i + 1, i))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + b"\n")


def read_fasta(path):
    names, seqs = [], []
    for ln in open(path):
        if ln.startswith(">"):
            names.append(ln.split()[0][1:])
            seqs.append([])
        else:
            seqs[-1].append(ln.strip())
    return names, ["".join(s) for s in seqs]


def kmer_dict(seqs):
    d = {}
    for s in seqs:
        b = s.encode() if isinstance(s, str) else bytes(s)
        for m in re.finditer(rb"[ACGT]{%d,}" % K, b.upper()):
            t = m.group()
            for i in range(len(t) - K + 1):
                km = t[i:i + K]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                d[key] = d.get(key, 0) + 1
    return d


def spectrum_cells(rd, ad):
    """{(row, column): distinct k-mers}, non-zero cells only"""
    cells = {}
    for key, c in rd.items():
        rc_ = (min(ad.get(key, 0), 5), min(c, 10001))
        cells[rc_] = cells.get(rc_, 0) + 1
    for key, m in ad.items():
        if key not in rd:
            rc_ = (min(m, 5), 0)
            cells[rc_] = cells.get(rc_, 0) + 1
    return cells


def cn_text(cells):
    return "#copies\tread_count\tkmers\n" + "".join("%s\t%d\t%d\n" % (LABELS[m], c, cells[(m, c)]) for m, c in sorted(cells))


def completeness_fields(stage, cells, thre):
    solid = sum(v for (m, c), v in cells.items() if c >= thre)
    found = sum(v for (m, c), v in cells.items() if c >= thre and m >= 1)
    distinct = sum(v for (m, c), v in cells.items() if m >= 1)
    only = sum(v for (m, c), v in cells.items() if m >= 1 and c == 0)
    return [stage, str(K), str(thre), str(solid), str(found), 100.0 * found / solid, str(distinct), str(only)]


def check_completeness(text, want_rows):
    """integers exactly, the percentage to 1e-4 (printed to four decimals)"""
    lines = text.splitlines()
    assert lines[0] == "#stage\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tasm_distinct\tasm_only"
    assert len(lines) == 1 + len(want_rows) and text.endswith("\n")
    for ln, want in zip(lines[1:], want_rows):
        f = ln.split("\t")
        assert f[:5] == want[:5] and f[6:] == want[6:], ln
        assert re.match(r"^\d+\.\d{4}$", f[5]) and abs(float(f[5]) - want[5]) <= 1e-4, ln


def cli(cwd, args, env=None, module="jasper_amd.cli"):
    p = subprocess.run([sys.executable, "-m", module] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def messages(stdout):
    return [ln.split("] ", 1)[1] for ln in stdout.splitlines() if re.match(r"^\[\w{3} \w{3} +\d", ln)]


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("spectra", ["--spectra"]), ("both", ["--spectra", "--report"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


def test_one_gpu_spectra_files_and_nothing_else_changes(runs):
    (d0, p0), (d1, p1) = runs["plain"], runs["spectra"]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    for fn in COMMON:
        assert os.path.isfile(d0 / fn), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "k-mer completeness" in m]
    assert [m for m in m1 if m not in extra] == m0                      # same log lines otherwise
    i = m1.index(extra[0])
    assert len(extra) == 2 and "After Polishing: Q value" in m1[i - 1] and m1[i + 1] == extra[1]      # right after the reference's two Q lines
    assert extra[0].startswith("Before Polishing: k-mer completeness = ") and extra[1].startswith("After Polishing: k-mer completeness = ")
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(SPECTRA_FILES)
    assert set(os.listdir(d0)) <= set(os.listdir(d1))
    # expected files from Python dicts
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    assert thre >= 1
    rd = kmer_dict(open(d1 / "reads.fq", "rb").read().split(b"\n")[1::4])
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["ctg1", "ctg2", "ctg3"] and pnames == names
    before, after = spectrum_cells(rd, kmer_dict(seqs)), spectrum_cells(rd, kmer_dict(pseqs))
    assert open(d1 / "asm.fa.spectra_cn.before.tsv").read() == cn_text(before)
    assert open(d1 / "asm.fa.spectra_cn.after.tsv").read() == cn_text(after)
    rows = [completeness_fields("before", before, thre), completeness_fields("after", after, thre)]
    text = open(d1 / "asm.fa.completeness.tsv").read()
    check_completeness(text, rows)
    # rows 0 .. 3 and the assembly-only column are there, and polishing removed assembly-only k-mers
    assert {m for m, c in before} >= {0, 1, 2, 3} and any(c == 0 for m, c in before)
    assert int(rows[1][7]) < int(rows[0][7])
    # the log lines carry the file's numbers
    got = [ln.split("\t") for ln in text.splitlines()[1:]]
    for line, f in zip(extra, got):
        assert line.endswith("= %s %% (%s of %s solid k-mers, threshold %s); %s assembly-only k-mers" % (f[5], f[4], f[3], f[2], f[7]))


def test_spectra_and_report_together_give_the_union(runs):
    (d0, _), (d1, _), (d2, p2) = runs["plain"], runs["spectra"], runs["both"]
    assert sorted(set(os.listdir(d2)) - set(os.listdir(d0))) == sorted(SPECTRA_FILES + REPORT_FILES)
    for fn in SPECTRA_FILES + COMMON:
        assert open(d2 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    m2 = messages(p2.stdout)
    assert len([m for m in m2 if "dense k-mer QV" in m]) == 2 and len([m for m in m2 if "k-mer completeness" in m]) == 2
    assert not [fn for fn in os.listdir(d2) if fn.endswith(".tmp")]


def test_two_ranks_on_one_gpu_give_the_same_spectra(runs, tmp_path):
    from test_gpu_cli_e2e import _torchrun_cli
    write_inputs(tmp_path)
    p = _torchrun_cli(tmp_path, ARGS + ["--spectra"])
    assert p.returncode == 0, p.stdout + p.stderr
    d1 = runs["spectra"][0]
    for fn in SPECTRA_FILES + ("asm.fa.polished.fasta",):
        assert open(tmp_path / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    assert len([m for m in messages(p.stdout) if "k-mer completeness" in m]) == 2          # only rank 0 talks


def test_kmerqc_spectra_reproduces_the_before_row(runs, tmp_path):
    d1 = runs["spectra"][0]
    thre = open(d1 / "threshold.txt").read().split()[0]
    seen = set(os.listdir(d1))
    p = cli(d1, ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", thre, "-o", str(tmp_path / "qc"), "--spectra"], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == ["qc.completeness.tsv", "qc.kmer_qv.tsv", "qc.spectra_cn.tsv", "qc.unreliable.bed"]
    driver = open(d1 / "asm.fa.completeness.tsv").read().splitlines()
    want = [driver[0], driver[1].replace("before\t", "asm\t", 1)]
    assert driver[1].startswith("before\t")
    assert open(tmp_path / "qc.completeness.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.spectra_cn.tsv").read() == open(d1 / "asm.fa.spectra_cn.before.tsv").read()
    assert len([m for m in messages(p.stdout) if "k-mer completeness" in m and "assembly-only k-mers" in m]) == 1
    # counting the reads and deriving the threshold as the driver does arrives at the same files
    cli(d1, ["--spectra", "-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "-o", str(tmp_path / "qr")], module="jasper_amd.kmerqc")
    assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("qr.")) == ["qr.completeness.tsv", "qr.kmer_qv.tsv", "qr.spectra_cn.tsv", "qr.unreliable.bed"]
    assert open(tmp_path / "qr.completeness.tsv").read() == open(tmp_path / "qc.completeness.tsv").read()
    assert open(tmp_path / "qr.spectra_cn.tsv").read() == open(tmp_path / "qc.spectra_cn.tsv").read()
    # without the flag the evaluator writes its two files only
    cli(d1, ["-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("q0.")) == ["q0.kmer_qv.tsv", "q0.unreliable.bed"]
    assert open(tmp_path / "q0.kmer_qv.tsv").read() == open(tmp_path / "qr.kmer_qv.tsv").read()
