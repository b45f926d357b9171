"""GPU: `python -m jasper_amd.cli ... --copies` and `python -m jasper_amd.kmerqc ... --copies` on a small synthetic case.

Without the flag nothing changes; with it the three new files equal what this file computes with Python dicts from reads.fq,
asm.fa and the polished FASTA it reads back (its own restatement of the semantics in include/jasper_hip.h and of the file
formats in README.md)."""
import os
import re

import pytest

from test_gpu_cli_spectra import ARGS, COMMON, K, REPORT_FILES, SPECTRA_FILES, cli, cn_text, kmer_dict, messages, read_fasta, spectrum_cells
from test_gpu_cli_spectra import write_inputs as write_spectra_inputs

pytestmark = pytest.mark.gpu
COPIES_FILES = ("asm.fa.copies.after.bed", "asm.fa.copies.before.bed", "asm.fa.copies.tsv")
TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\texcess\tdeficit\tsum_reads\tsum_asm\tdepth\tpeak"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


ALL_PEAK, ALL_MIN_RUN = 40, 2      # the flags of the run with every extension


def write_inputs(d):
    """the spectra test's three contigs (ctg3 repeats a piece of ctg1 once and a piece of ctg2 twice: duplicated sequence), and
    reads that cover 1200 bases of ctg1 twice more (error-free, every second position): a collapsed repeat"""
    write_spectra_inputs(d)
    seq = read_fasta(d / "asm.fa")[1][0][5000:6200].upper()
    with open(d / "reads.fq", "ab") as f:
        for i in range(0, len(seq) - 150 + 1, 2):
            f.write(b"@x%d\n" % i + seq[i:i + 150].encode() + b"\n+\n" + b"I" * 150 + b"\n")


def peak_rule(h, thre):
    best, best_n = None, 0
    for c in range(max(thre, 2), 10001):
        if h.get(c, 0) > best_n:
            best, best_n = c, h[c]
    return best


def scan(seqs, rd, ad, thre, peak):
    """per sequence the six counters and the runs (seq, start, n_kmers, kind, sum_reads, sum_asm) of the semantics in jasper_hip.h"""
    counts, runs = [], []
    for si, s in enumerate(seqs):
        b = s.encode()
        up = b.upper()
        valid = ex = de = sr = sa = 0
        cur = None
        bad = [ch not in b"ACGTacgt" for ch in b]
        nbad = sum(bad[:K - 1])
        for i in range(max(0, len(b) - K + 1)):
            nbad += bad[i + K - 1]
            cls = 0
            if nbad == 0:
                km = up[i:i + K]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                c, a = rd.get(key, 0), ad.get(key, 0)
                valid += 1
                sr += c
                sa += a
                if c >= thre:
                    e = (2 * c + peak) // (2 * peak)
                    cls = 1 if e > a else 2 if e < a else 0
                ex += cls == 1
                de += cls == 2
            nbad -= bad[i]
            if cur is not None and cur[3] != cls:
                runs.append(tuple(cur))
                cur = None
            if cls:
                if cur is None:
                    cur = [si, i, 0, cls, 0, 0]
                cur[2] += 1
                cur[4] += c
                cur[5] += a
        if cur is not None:
            runs.append(tuple(cur))
        counts.append((max(0, len(b) - K + 1), valid, ex, de, sr, sa))
    return counts, runs


def tsv_rows(names, stage, seqs, counts, peak):
    """{(contig, stage): fields} with the depth as a float (or "NA")"""
    rows = {}
    tot = [0] * 7
    for n, s, c in zip(names, seqs, counts):
        rows[(n, stage)] = [len(s)] + list(c)
        tot = [x + y for x, y in zip(tot, [len(s)] + list(c))]
    rows[("*", stage)] = tot
    return {key: [str(v) for v in f] + [f[5] / (peak * f[6]) if f[6] else "NA", str(peak)] for key, f in rows.items()}


def check_tsv(text, want, order):
    """integers exactly, the depth to 1e-4 (printed to four decimals), rows in the given order"""
    lines = text.splitlines()
    assert lines[0] == TSV_HEADER and text.endswith("\n") and len(lines) == 1 + len(order)
    for ln, key in zip(lines[1:], order):
        f = ln.split("\t")
        w = want[key]
        assert tuple(f[:2]) == key and f[2:9] == w[:7] and f[10] == w[8], ln
        if w[7] == "NA":
            assert f[9] == "NA", ln
        else:
            assert re.match(r"^\d+\.\d{4}$", f[9]) and abs(float(f[9]) - w[7]) <= 1e-4, ln


def check_bed(text, names, runs, peak, min_run):
    lines = text.splitlines()
    want = [r for r in runs if r[2] >= min_run]
    assert len(lines) == len(want) and (text.endswith("\n") or not want)
    for ln, (seq, start, nk, kind, sr, sa) in zip(lines, want):
        f = ln.split("\t")
        assert f[:5] == [names[seq], str(start), str(start + nk + K - 1), ("excess", "deficit")[kind - 1], str(nk)], ln
        for got, val in zip(f[5:], (sr / nk, sa / nk, sr / (peak * nk))):
            assert re.match(r"^\d+\.\d{2}$", got) and abs(float(got) - val) <= 0.005 + 1e-9, ln
    return want


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("copies", ["--copies"]), ("all", ["--copies", "--spectra", "--report", "--peak", str(ALL_PEAK), "--copies-min-run", str(ALL_MIN_RUN)])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    """the dicts and the expected scans of the `copies` run"""
    d1 = runs["copies"][0]
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    rd = kmer_dict(open(d1 / "reads.fq", "rb").read().split(b"\n")[1::4])
    h = {}
    for c in rd.values():
        h[min(c, 10001)] = h.get(min(c, 10001), 0) + 1
    peak = peak_rule(h, thre)
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["ctg1", "ctg2", "ctg3"] and pnames == names and thre >= 1 and peak > thre
    return dict(thre=thre, peak=peak, rd=rd, names=names, seqs=seqs, pseqs=pseqs, ad0=kmer_dict(seqs), ad1=kmer_dict(pseqs))


def test_one_gpu_copies_files_and_nothing_else_changes(runs, truth):
    (d0, p0), (d1, p1) = runs["plain"], runs["copies"]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    for fn in COMMON:
        assert os.path.isfile(d0 / fn), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "Copy-number scan" in m]
    assert [m for m in m1 if m not in extra] == m0                      # same log lines otherwise
    i = m1.index(extra[0])
    assert len(extra) == 2 and "After Polishing: Q value" in m1[i - 1] and m1[i + 1] == extra[1]      # right after the reference's two Q lines
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(COPIES_FILES)
    assert set(os.listdir(d0)) <= set(os.listdir(d1))
    # expected files from Python dicts
    t = truth
    names, peak, thre = t["names"], t["peak"], t["thre"]
    c0, r0 = scan(t["seqs"], t["rd"], t["ad0"], thre, peak)
    c1, r1 = scan(t["pseqs"], t["rd"], t["ad1"], thre, peak)
    want = {**tsv_rows(names, "before", t["seqs"], c0, peak), **tsv_rows(names, "after", t["pseqs"], c1, peak)}
    order = [(n, s) for n in names for s in ("before", "after")] + [("*", "before"), ("*", "after")]
    check_tsv(open(d1 / "asm.fa.copies.tsv").read(), want, order)
    l0 = check_bed(open(d1 / "asm.fa.copies.before.bed").read(), names, r0, peak, K)      # --copies-min-run defaults to k
    l1 = check_bed(open(d1 / "asm.fa.copies.after.bed").read(), names, r1, peak, K)
    # the workload holds what the scan is for: the pieces ctg3 repeats are deficit, the stretch of ctg1 the reads cover three times is
    # excess, both kinds are listed, short runs are not
    assert c0[2][3] > 2000 and c0[0][2] > 800 and {r[3] for r in l0} == {1, 2}
    assert any(r[0] == 0 and r[3] == 1 and 5000 <= r[1] and r[1] + r[2] + K - 1 <= 6200 and r[2] >= 100 for r in l0)
    assert len(l0) < len(r0) and len(l1) < len(r1)
    assert extra[0] == "Copy-number scan: single-copy read count (peak) is %d (from the k-mer histogram)" % peak
    assert extra[1] == "Copy-number scan: before polishing %d excess and %d deficit windows, %d runs listed; after polishing %d excess and %d deficit windows, %d runs listed" % (
        sum(c[2] for c in c0), sum(c[3] for c in c0), len(l0), sum(c[2] for c in c1), sum(c[3] for c in c1), len(l1))


def test_copies_spectra_and_report_together_give_the_union(runs, truth):
    """... with --peak and --copies-min-run given: the files are those of the dicts for that peak, every run of 2 windows or more listed"""
    (d0, _), (d1, _), (d2, p2) = runs["plain"], runs["copies"], runs["all"]
    assert sorted(set(os.listdir(d2)) - set(os.listdir(d0))) == sorted(COPIES_FILES + SPECTRA_FILES + REPORT_FILES)
    for fn in COMMON:
        assert open(d2 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    t = truth
    names = t["names"]
    c0, r0 = scan(t["seqs"], t["rd"], t["ad0"], t["thre"], ALL_PEAK)
    c1, r1 = scan(t["pseqs"], t["rd"], t["ad1"], t["thre"], ALL_PEAK)
    want = {**tsv_rows(names, "before", t["seqs"], c0, ALL_PEAK), **tsv_rows(names, "after", t["pseqs"], c1, ALL_PEAK)}
    check_tsv(open(d2 / "asm.fa.copies.tsv").read(), want, [(n, s) for n in names for s in ("before", "after")] + [("*", "before"), ("*", "after")])
    l0 = check_bed(open(d2 / "asm.fa.copies.before.bed").read(), names, r0, ALL_PEAK, ALL_MIN_RUN)
    l1 = check_bed(open(d2 / "asm.fa.copies.after.bed").read(), names, r1, ALL_PEAK, ALL_MIN_RUN)
    assert ALL_PEAK != t["peak"] and len(l0) > len([r for r in r0 if r[2] >= K]) and len(l1) > 0
    # the assembly's table is counted once per stage and serves both: the spectrum's files are what the dicts give
    assert open(d2 / "asm.fa.spectra_cn.before.tsv").read() == cn_text(spectrum_cells(t["rd"], t["ad0"]))
    assert open(d2 / "asm.fa.spectra_cn.after.tsv").read() == cn_text(spectrum_cells(t["rd"], t["ad1"]))
    m2 = messages(p2.stdout)
    assert [sum(what in m for m in m2) for what in ("dense k-mer QV", "k-mer completeness", "Copy-number scan")] == [2, 2, 2]
    assert "Copy-number scan: single-copy read count (peak) is %d (given by --peak)" % ALL_PEAK in m2
    ix = [min(i for i, m in enumerate(m2) if what in m) for what in ("dense k-mer QV", "k-mer completeness", "Copy-number scan", "Polished sequence is in")]
    assert ix == sorted(ix)                                                # the new lines come after the existing ones
    assert not [fn for fn in os.listdir(d2) if fn.endswith(".tmp")]


def test_two_ranks_on_one_gpu_give_the_same_files(runs, tmp_path):
    from test_gpu_cli_e2e import _torchrun_cli
    write_inputs(tmp_path)
    p = _torchrun_cli(tmp_path, ARGS + ["--copies"])
    assert p.returncode == 0, p.stdout + p.stderr
    d1 = runs["copies"][0]
    for fn in COPIES_FILES + ("asm.fa.polished.fasta",):
        assert open(tmp_path / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    assert len([m for m in messages(p.stdout) if "Copy-number scan" in m]) == 2            # only rank 0 talks


def test_kmerqc_copies_reproduces_the_before_rows(runs, truth, tmp_path):
    d1 = runs["copies"][0]
    thre = str(truth["thre"])
    seen = set(os.listdir(d1))
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", thre]
    p = cli(d1, base + ["-o", str(tmp_path / "qc"), "--copies"], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == ["qc.copies.bed", "qc.copies.tsv", "qc.kmer_qv.tsv", "qc.unreliable.bed"]
    driver = open(d1 / "asm.fa.copies.tsv").read().splitlines()
    want = [driver[0]] + [ln.replace("\tbefore\t", "\tasm\t", 1) for ln in driver[1:] if "\tbefore\t" in ln]
    assert len(want) == 5 and open(tmp_path / "qc.copies.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.copies.bed").read() == open(d1 / "asm.fa.copies.before.bed").read()
    assert len([m for m in messages(p.stdout) if "Copy-number scan" in m]) == 1
    # --peak overrides the histogram's, --copies-min-run 1 lists every run; --spectra beside it changes nothing
    peak2 = truth["peak"] + 7
    cli(d1, base + ["-o", str(tmp_path / "qp"), "--copies", "--peak", str(peak2), "--copies-min-run", "1", "--spectra"], module="jasper_amd.kmerqc")
    assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("qp.")) == ["qp.completeness.tsv", "qp.copies.bed", "qp.copies.tsv", "qp.kmer_qv.tsv",
                                                                                 "qp.spectra_cn.tsv", "qp.unreliable.bed"]
    c0, r0 = scan(truth["seqs"], truth["rd"], truth["ad0"], truth["thre"], peak2)
    check_tsv(open(tmp_path / "qp.copies.tsv").read(), tsv_rows(truth["names"], "asm", truth["seqs"], c0, peak2), [(n, "asm") for n in truth["names"] + ["*"]])
    assert len(check_bed(open(tmp_path / "qp.copies.bed").read(), truth["names"], r0, peak2, 1)) == len(r0) > 0
    assert open(tmp_path / "qp.kmer_qv.tsv").read() == open(tmp_path / "qc.kmer_qv.tsv").read()
    assert open(tmp_path / "qp.spectra_cn.tsv").read() == open(runs["all"][0] / "asm.fa.spectra_cn.before.tsv").read()


def test_a_histogram_without_a_peak_and_no_peak_given_exits_1(runs, tmp_path):
    import subprocess
    import sys
    from test_gpu_cli_spectra import ROOT
    d1 = runs["copies"][0]
    args = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", "10001", "-o", str(tmp_path / "q"), "--copies"]      # no bin from 10001 to 10000
    p = subprocess.run([sys.executable, "-m", "jasper_amd.kmerqc"] + args, cwd=d1, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "--peak" in p.stderr and os.listdir(tmp_path) == []
    cli(d1, args + ["--peak", "30"], module="jasper_amd.kmerqc")           # the same with --peak goes through
    assert sorted(os.listdir(tmp_path)) == ["q.copies.bed", "q.copies.tsv", "q.kmer_qv.tsv", "q.unreliable.bed"]
    for bad in (["--peak", "0"], ["--copies-min-run", "none"]):
        p = subprocess.run([sys.executable, "-m", "jasper_amd.cli"] + ARGS + ["--copies"] + bad, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 1 and "--peak and --copies-min-run" in p.stderr
