"""GPU: `python -m jasper_amd.cli ... --dups` and `python -m jasper_amd.kmerqc ... --dups` on a small synthetic case: three contigs,
the third a copy of 5 kb of the first with three planted substitutions, reads sampled from the genome without that copy.

Without the flag nothing changes; with it the four new files equal what this file computes with the restatement of
tests/test_gpu_dups.py from reads.fq, asm.fa and the polished FASTA it reads back, and the file formats of README.md written out here
again.  --copies beside it writes byte for byte what --copies alone writes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cli_spectra import COMMON, ROOT, cli, messages, read_fasta
from test_gpu_dups import count_dict, restate

pytestmark = pytest.mark.gpu
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
DUPS_FILES = ("asm.fa.dups.after.bed", "asm.fa.dups.before.bed", "asm.fa.dups.pairs.tsv", "asm.fa.dups.tsv")
COPIES_FILES = ("asm.fa.copies.after.bed", "asm.fa.copies.before.bed", "asm.fa.copies.tsv")
TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\ttwo_copy\tdeficit\tmulti\tunplaced\tread_copies\tbest_mate\tbest_windows\tbest_fraction"
PAIRS_HEADER = "#stage\tcontig\tmate\tstrand\truns\twindows\tdeficit\tread_copies"
SUBS = (1200, 2600, 4100)       # where ctg3 differs from the piece of ctg1 it copies


def write_inputs(d):
    from jasper_amd import synth
    rng = np.random.default_rng(47)
    genome = synth.make_genome(rng, 40_000, repeat_frac=0)      # (no planted repeats: the copy is the only duplication)
    reads = synth.make_reads_stream(rng, genome, 30, 150, 0.003).reshape(-1, 151)[:, :150]
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + b"I" * 150 + b"\n")
    asm = synth.make_assembly(rng, genome, err=3e-3, n_every=17_000, n_len=30).tobytes()
    ctg1, ctg2 = asm[:18_000], asm[18_000:]
    copy = bytearray(ctg1[6000:11_000])
    for p in SUBS:
        copy[p:p + 1] = b"ACGT"[(b"ACGT".index(copy[p:p + 1].upper()) + 1) % 4:][:1]
    with open(d / "asm.fa", "wb") as f:
        for name, s in (("ctg1", ctg1), ("ctg2", ctg2), ("ctg3", bytes(copy))):
            f.write(b">" + name.encode() + b" synthetic\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + b"\n")


def peak_rule(h, thre):
    best, best_n = None, 0
    for c in range(max(thre, 2), 10001):
        if h.get(c, 0) > best_n:
            best, best_n = c, h[c]
    return best


def near(text, value, decimals):
    return re.match(r"^\d+\.\d{%d}$" % decimals, text) and abs(float(text) - value) <= 0.5 * 10 ** -decimals + 1e-9


def check_tsv(text, names, stages, peak):
    """stages: [(stage, lengths, counts, runs)]; integers and names exactly, the two ratios to their printed precision"""
    lines = text.splitlines()
    assert lines[0] == TSV_HEADER and text.endswith("\n") and len(lines) == 1 + (len(names) + 1) * len(stages)
    want = {}
    for stage, lengths, counts, runs in stages:
        tot = [0] * 9
        for i, n in enumerate(names):
            per = {}
            for r in runs:
                if r[0] == i:
                    per[r[3]] = per.get(r[3], 0) + r[2]
            best = min(per, key=lambda m: (-per[m], m)) if per else None
            row = [lengths[i]] + list(counts[i]) + [per[best] if per else 0]
            want[(n, stage)] = row + [names[best] if per else "."]
            tot = [a + b for a, b in zip(tot, row)]
        want[("*", stage)] = tot + ["."]
    order = [(n, s[0]) for n in names for s in stages] + [("*", s[0]) for s in stages]
    for ln, key in zip(lines[1:], order):
        f = ln.split("\t")
        length, w, v, two, de, mu, un, sr, bw, best = want[key]
        assert tuple(f[:2]) == key and f[2:9] == [str(x) for x in (length, w, v, two, de, mu, un)] and f[10:12] == [best, str(bw)], ln
        assert f[9] == "NA" if two == 0 else near(f[9], sr / (peak * two), 2), ln
        assert f[12] == "NA" if v == 0 else near(f[12], bw / v, 4), ln


def check_bed(text, names, runs, peak, min_run):
    lines = text.splitlines()
    want = [r for r in runs if r[2] >= min_run]
    assert len(lines) == len(want) and (text.endswith("\n") or not want)
    for ln, (seq, start, nk, mseq, mstart, strand, sr, nd) in zip(lines, want):
        f = ln.split("\t")
        assert f[:8] == [names[seq], str(start), str(start + nk + K - 1), names[mseq], str(mstart), str(mstart + nk + K - 1), "+-"[strand], str(nk)], ln
        assert near(f[8], sr / (peak * nk), 2) and near(f[9], nd / nk, 4) and len(f) == 10, ln
    return want


def check_pairs(text, stages, peak):
    """stages: [(stage, names, runs)]; runs of every length count"""
    lines = text.splitlines()
    assert lines[0] == PAIRS_HEADER and text.endswith("\n")
    want = []
    for stage, names, runs in stages:
        d = {}
        for seq, _, nk, mseq, _, strand, sr, nd in runs:
            p = d.setdefault((seq, mseq, strand), [0, 0, 0, 0])
            p[0], p[1], p[2], p[3] = p[0] + 1, p[1] + nk, p[2] + nd, p[3] + sr
        want += [(stage, names[key[0]], names[key[1]], "+-"[key[2]], d[key]) for key in sorted(d)]
    assert len(lines) == 1 + len(want)
    for ln, (stage, a, b, strand, (nr, nw, nd, sr)) in zip(lines[1:], want):
        f = ln.split("\t")
        assert f[:7] == [stage, a, b, strand, str(nr), str(nw), str(nd)] and near(f[7], sr / (peak * nw), 2) and len(f) == 8, ln
    return want


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("dups", ["--dups"]), ("copies", ["--copies"]), ("both", ["--copies", "--dups", "--dups-min-run", "1"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d1 = runs["dups"][0]
    thre = int(open(d1 / "threshold.txt").read().split()[0])
    rd = count_dict([(ln, 1) for ln in open(d1 / "reads.fq", "rb").read().split(b"\n")[1::4]], K)
    h = {}
    for c in rd.values():
        h[min(c, 10001)] = h.get(min(c, 10001), 0) + 1
    peak = peak_rule(h, thre)
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["ctg1", "ctg2", "ctg3"] and pnames == names and thre >= 1 and peak > thre
    seqs, pseqs = [s.encode() for s in seqs], [s.encode() for s in pseqs]
    return dict(thre=thre, peak=peak, rd=rd, names=names, seqs=seqs, pseqs=pseqs, before=restate(seqs, K, rd, thre, peak), after=restate(pseqs, K, rd, thre, peak))


def test_one_gpu_dups_files_and_nothing_else_changes(runs, truth):
    (d0, p0), (d1, p1) = runs["copies"], runs["dups"]
    for fn in COMMON:
        assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    assert not [fn for fn in os.listdir(d0) if ".dups." in fn]                  # without --dups no dups file appears
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(DUPS_FILES) and not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "Duplication map" in m]
    assert [m for m in m1 if m not in extra] == [m for m in m0 if "Copy-number scan" not in m]      # same log lines otherwise
    t = truth
    names, peak = t["names"], t["peak"]
    (c0, r0), (c1, r1) = t["before"], t["after"]
    check_tsv(open(d1 / "asm.fa.dups.tsv").read(), names, [("before", [len(s) for s in t["seqs"]], c0, r0), ("after", [len(s) for s in t["pseqs"]], c1, r1)], peak)
    l0 = check_bed(open(d1 / "asm.fa.dups.before.bed").read(), names, r0, peak, K)      # --dups-min-run defaults to k
    l1 = check_bed(open(d1 / "asm.fa.dups.after.bed").read(), names, r1, peak, K)
    pairs = check_pairs(open(d1 / "asm.fa.dups.pairs.tsv").read(), [("before", names, r0), ("after", names, r1)], peak)
    # the workload holds what the map is for: ctg3 pairs with ctg1 in four runs cut by the three substitutions, k windows apart on one
    # diagonal, the reads support one copy of the two (deficit), and ctg2 takes no part
    mine = [r for r in l0 if r[0] == 2]
    assert len(mine) == 4 and all(r[3] == 0 and r[5] == 0 and r[4] - r[1] == 6000 for r in mine)
    assert [b[1] - (a[1] + a[2]) for a, b in zip(mine, mine[1:])] == [K, K, K] and [r[1] + r[2] - 1 for r in mine[:3]] == [p - K for p in SUBS]
    assert c0[2][2] >= 5000 - K + 1 - 3 * K and c0[2][3] > 0.75 * c0[2][2] and c0[1][2] == 0 and c0[0][5] == c0[2][5] == 0
    assert ("before", "ctg3", "ctg1", "+") in [p[:4] for p in pairs] and ("before", "ctg1", "ctg3", "+") in [p[:4] for p in pairs]
    assert extra == ["Duplication map: single-copy read count (peak) is %d (from the k-mer histogram)" % peak,
                     "Duplication map: before polishing %s; after polishing %s" % tuple(
                         "%d two-copy, %d deficit, %d multi and %d unplaced windows, %d runs listed" % (tuple(sum(c[i] for c in cs) for i in (2, 3, 4, 5)) + (len(ls),))
                         for cs, ls in ((c0, l0), (c1, l1)))]
    last = [i for i, m in enumerate(m1) if "Polished sequence is in" in m]
    assert len(last) == 1 and m1.index(extra[0]) + 1 == m1.index(extra[1]) < last[0] and max(i for i, m in enumerate(m1) if "Q value" in m) < m1.index(extra[0])


def test_copies_beside_dups_is_what_copies_alone_writes(runs, truth):
    (d0, _), (d2, p2) = runs["copies"], runs["both"]
    for fn in COPIES_FILES + COMMON:
        assert open(d2 / fn, "rb").read() == open(d0 / fn, "rb").read(), fn
    assert sorted(set(os.listdir(d2)) - set(os.listdir(d0))) == sorted(DUPS_FILES)
    t = truth
    (c0, r0), (c1, r1) = t["before"], t["after"]
    assert len(check_bed(open(d2 / "asm.fa.dups.before.bed").read(), t["names"], r0, t["peak"], 1)) == len(r0)      # --dups-min-run 1 lists every run
    check_bed(open(d2 / "asm.fa.dups.after.bed").read(), t["names"], r1, t["peak"], 1)
    assert open(d2 / "asm.fa.dups.pairs.tsv").read() == open(runs["dups"][0] / "asm.fa.dups.pairs.tsv").read()       # (the filter is the BED's alone)
    assert open(d2 / "asm.fa.dups.tsv").read() == open(runs["dups"][0] / "asm.fa.dups.tsv").read()
    m2 = messages(p2.stdout)
    ix = [min(i for i, m in enumerate(m2) if what in m) for what in ("Copy-number scan", "Duplication map", "Polished sequence is in")]
    assert ix == sorted(ix) and [sum(what in m for m in m2) for what in ("Copy-number scan", "Duplication map")] == [2, 1]


def test_kmerqc_dups_reproduces_the_before_rows(runs, truth, tmp_path):
    d1 = runs["dups"][0]
    seen = set(os.listdir(d1))
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(truth["thre"])]
    p = cli(d1, base + ["-o", str(tmp_path / "qc"), "--dups"], module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == ["qc.dups.bed", "qc.dups.pairs.tsv", "qc.dups.tsv", "qc.kmer_qv.tsv", "qc.unreliable.bed"]
    driver = open(d1 / "asm.fa.dups.tsv").read().splitlines()
    want = [driver[0]] + [ln.replace("\tbefore\t", "\tasm\t", 1) for ln in driver[1:] if "\tbefore\t" in ln]
    assert len(want) == 5 and open(tmp_path / "qc.dups.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.dups.bed").read() == open(d1 / "asm.fa.dups.before.bed").read()
    pairs = open(d1 / "asm.fa.dups.pairs.tsv").read().splitlines()
    assert open(tmp_path / "qc.dups.pairs.tsv").read().splitlines() == [pairs[0]] + [ln.replace("before\t", "asm\t", 1) for ln in pairs[1:] if ln.startswith("before\t")]
    assert len([m for m in messages(p.stdout) if "Duplication map" in m]) == 1


def test_flag_errors_exit_1_with_a_message(runs, tmp_path):
    d1 = runs["dups"][0]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for module, args in (("jasper_amd.cli", ARGS), ("jasper_amd.kmerqc", ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "-o", str(tmp_path / "q")])):
        for bad, msg in ((["--dups-min-run", "5"], "give --dups as well"), (["--dups", "--dups-min-run", "0"], "--dups-min-run takes an integer of at least 1"),
                         (["--dups", "--peak", "0"], "--peak")):
            p = subprocess.run([sys.executable, "-m", module] + args + bad, cwd=d1, env=env, capture_output=True, text=True, timeout=600)
            assert p.returncode == 1 and msg in p.stdout + p.stderr, (module, bad, p.stdout, p.stderr)
    # a histogram without a peak and no --peak: the message and the status of --copies
    args = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", "10001", "-o", str(tmp_path / "q"), "--dups"]
    p = subprocess.run([sys.executable, "-m", "jasper_amd.kmerqc"] + args, cwd=d1, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "--peak" in p.stderr and os.listdir(tmp_path) == []
