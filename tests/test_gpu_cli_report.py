"""GPU: `python -m jasper_amd.cli ... --report` and `python -m jasper_amd.kmerqc` on a small synthetic case.

Without the flag nothing changes; with it the three report files equal what this file computes with oracle.OracleDB from the
input FASTA and from the polished FASTA it reads back (its own restatement of the semantics in include/jasper_hip.h and of
the file formats in README.md)."""
import math
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
REPORT_FILES = ("asm.fa.kmer_qv.tsv", "asm.fa.unreliable.before.bed", "asm.fa.unreliable.after.bed")
U32 = 2**32 - 1


def write_inputs(d):
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


def dense(odb, seq, thre):
    """(windows, valid, unreliable, absent), [(start, n_kmers, n_absent, min_count)] of one sequence"""
    b = seq.encode()
    n = len(b)
    up = b.upper()
    valid = unrel = absent = 0
    runs, cur = [], None
    bad_until = -1
    for i in range(n):
        if b[i] not in b"ACGTacgt":
            bad_until = i
        w = i - K + 1                                   # the window that ends at i
        if w < 0:
            continue
        c = min(odb.query(up[w:w + K]), U32) if bad_until < w else None
        if c is not None:
            valid += 1
            absent += c == 0
        if c is not None and c < thre:
            unrel += 1
            if cur is None:
                cur = [w, 0, 0, c]
            cur[1] += 1
            cur[2] += c == 0
            cur[3] = min(cur[3], c)
        elif cur is not None:
            runs.append(tuple(cur))
            cur = None
    if cur is not None:
        runs.append(tuple(cur))
    return (max(0, n - K + 1), valid, unrel, absent), runs


def qv(x, valid):
    if valid == 0:
        return "NA"
    if x == 0:
        return "inf"
    return -10 * math.log10(1 - (1 - x / valid) ** (1 / K))


def bed_lines(names, runs_per_seq):
    out = []
    for name, runs in zip(names, runs_per_seq):
        for start, nk, na, mn in runs:
            cs, ce = (start + nk - 1, start + K) if nk <= K else (start, start)
            out.append("\t".join([name] + [str(v) for v in (start, start + nk + K - 1, nk, na, mn, cs, ce)]) + "\n")
    return "".join(out)


def check_tsv(text, want_rows):
    """want_rows: [(contig, stage, length, (windows, valid, unreliable, absent))]; integers exactly, QV to 1e-3 (printed to four decimals)"""
    lines = text.splitlines()
    assert lines[0] == "#contig\tstage\tlength\twindows\tvalid\tunreliable\tabsent\tQV_unreliable\tQV_absent"
    assert len(lines) == 1 + len(want_rows)
    for ln, (name, stage, length, c) in zip(lines[1:], want_rows):
        f = ln.split("\t")
        assert f[:7] == [name, stage, str(length)] + [str(v) for v in c], ln
        for got, want in zip(f[7:], (qv(c[2], c[1]), qv(c[3], c[1]))):
            if isinstance(want, str):
                assert got == want, ln
            else:
                assert re.match(r"^-?\d+\.\d{4}$", got) and abs(float(got) - want) <= 1e-3, ln


def cli(cwd, args, env=None, module="jasper_amd.cli"):
    p = subprocess.run([sys.executable, "-m", module] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def messages(stdout):
    return [ln.split("] ", 1)[1] for ln in stdout.splitlines() if re.match(r"^\[\w{3} \w{3} +\d", ln)]


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode in ("plain", "report"):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + (["--report"] if mode == "report" else [])))
    return out


def test_one_gpu_report_files_and_nothing_else_changes(runs):
    from oracle import oracle as O
    (d0, p0), (d1, p1) = runs["plain"], runs["report"]
    for fn in ("asm.fa.polished.fasta", "asm.fa.fixes.csv", "jfhisto%d.csv" % K, "threshold.txt"):
        assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    assert [m for m in m0 if "Q value" in m] == [m for m in m1 if "Q value" in m] and len([m for m in m0 if "Q value" in m]) == 2
    extra = [m for m in m1 if "dense k-mer QV" in m]
    assert [m for m in m1 if m not in extra] == m0                      # same log lines otherwise
    i = m1.index(extra[0])
    assert len(extra) == 2 and "After Polishing: Q value" in m1[i - 1] and m1[i + 1] == extra[1]      # right after the reference's two Q lines
    assert extra[0].startswith("Before Polishing: dense k-mer QV = ") and extra[1].startswith("After Polishing: dense k-mer QV = ")
    assert not any(os.path.exists(d0 / fn) for fn in REPORT_FILES)
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(REPORT_FILES)
    # expected files from the oracle's counts
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    odb = O.OracleDB(K)
    odb.count_text(open(d1 / "reads.fq", "rb").read())
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["ctg1", "ctg2", "ctg3"] and pnames == names
    before = [dense(odb, s, thre) for s in seqs]
    after = [dense(odb, s, thre) for s in pseqs]
    rows = []
    for i, n in enumerate(names):
        rows.append((n, "before", len(seqs[i]), before[i][0]))
        rows.append((n, "after", len(pseqs[i]), after[i][0]))
    for stage, res, ss in (("before", before, seqs), ("after", after, pseqs)):
        rows.append(("*", stage, sum(len(s) for s in ss), tuple(sum(r[0][j] for r in res) for j in range(4))))
    check_tsv(open(d1 / REPORT_FILES[0]).read(), rows)
    assert open(d1 / REPORT_FILES[1]).read() == bed_lines(names, [r[1] for r in before])
    assert open(d1 / REPORT_FILES[2]).read() == bed_lines(pnames, [r[1] for r in after])
    assert sum(len(r[1]) for r in before) >= 20 and sum(r[0][2] for r in after) < sum(r[0][2] for r in before)
    # the log lines carry the `*` rows' QVs
    star = [ln.split("\t") for ln in open(d1 / REPORT_FILES[0]).read().splitlines() if ln.startswith("*\t")]
    assert extra[0].endswith("= %s (unreliable k-mers), %s (absent k-mers)" % (star[0][7], star[0][8]))
    assert extra[1].endswith("= %s (unreliable k-mers), %s (absent k-mers)" % (star[1][7], star[1][8]))


def test_two_ranks_on_one_gpu_give_the_same_report(runs, tmp_path):
    from test_gpu_cli_e2e import _torchrun_cli
    write_inputs(tmp_path)
    p = _torchrun_cli(tmp_path, ARGS + ["--report"])
    assert p.returncode == 0, p.stdout + p.stderr
    d1 = runs["report"][0]
    for fn in REPORT_FILES + ("asm.fa.polished.fasta",):
        assert open(tmp_path / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    assert len([m for m in messages(p.stdout) if "dense k-mer QV" in m]) == 2          # only rank 0 talks


def test_python_assembly_route_gives_the_same_report(runs, tmp_path):
    write_inputs(tmp_path)
    cli(tmp_path, ARGS + ["--report"], env={"JASPER_AMD_NO_NATIVE_ASM": "1"})
    d1 = runs["report"][0]
    for fn in REPORT_FILES + ("asm.fa.polished.fasta",):
        assert open(tmp_path / fn, "rb").read() == open(d1 / fn, "rb").read(), fn


def test_kmerqc_reproduces_the_after_rows(runs, tmp_path):
    d1 = runs["report"][0]
    thre = open(d1 / "threshold.txt").read().split()[0]
    before = set(os.listdir(d1))
    cli(d1, ["-a", "asm.fa.polished.fasta", "-j", "mer_counts%d.jf" % K, "--threshold", thre, "-o", str(tmp_path / "qc")], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == before and sorted(os.listdir(tmp_path)) == ["qc.kmer_qv.tsv", "qc.unreliable.bed"]
    tsv = open(d1 / REPORT_FILES[0]).read().splitlines()
    want = [tsv[0]] + [ln.replace("\tafter\t", "\tasm\t") for ln in tsv[1:] if "\tafter\t" in ln]
    assert open(tmp_path / "qc.kmer_qv.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.unreliable.bed").read() == open(d1 / REPORT_FILES[2]).read()
    # counting the reads and deriving the threshold as the driver does arrives at the same files
    cli(d1, ["-a", "asm.fa.polished.fasta", "-r", "reads.fq", "-k", str(K), "-o", str(tmp_path / "qr")], module="jasper_amd.kmerqc")
    assert open(tmp_path / "qr.kmer_qv.tsv").read().splitlines() == want
    assert open(tmp_path / "qr.unreliable.bed").read() == open(d1 / REPORT_FILES[2]).read()
