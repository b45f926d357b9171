"""GPU: `python -m jasper_amd.kmerqc -a asm.fa --alt alt.fa ...` on a small synthetic diploid case.

Without --alt the evaluator writes the files it always wrote; with it the five new files equal what this file computes with Python dicts
from reads.fq, asm.fa and alt.fa (the semantics of include/jasper_hip.h as tests/test_gpu_diploid.py restates them, the file formats of
README.md as restated here), every other file is byte for byte the run's without --alt, and swapping the two haplotypes swaps the rows."""
import math
import os
import re

import numpy as np
import pytest

from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_diploid import kmer_dict, restate_pair, restate_scan

pytestmark = pytest.mark.gpu
K = 25
THRE = 5
CLASSES = ("reads_only", "asm_only", "alt_only", "shared")
PLAIN_FILES = ["p.completeness.tsv", "p.kmer_qv.tsv", "p.spectra_cn.tsv", "p.unreliable.bed"]
NEW_FILES = ["p.diploid.completeness.tsv", "p.diploid.tsv", "p.private.alt.bed", "p.private.asm.bed", "p.spectra_asm.tsv"]


def other_base(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


def write_inputs(d):
    """genome G and H = G with 40 SNPs and one deletion of 9 bases; error-free reads from both (20x each); asm.fa from G in two contigs (a
    stretch of the second in lower case, an N gap in the first) with five wrong bases, alt.fa from H in one contig with four; one of the
    wrong bases is in both"""
    from jasper_amd import synth
    rng = np.random.default_rng(47)
    G = synth.make_genome(rng, 30_000, repeat_frac=0)
    H = bytearray(G.tobytes())
    for p in sorted(rng.choice(np.arange(200, 29_800), size=40, replace=False).tolist()):
        H[p] = other_base(H[p])
    del H[15_000:15_009]
    Hn = np.frombuffer(bytes(H), dtype=np.uint8)
    with open(d / "reads.fq", "wb") as f:
        i = 0
        for genome in (G, Hn):
            for r in synth.make_reads_stream(rng, genome, 20, 150, 0.0).reshape(-1, 151)[:, :150]:
                f.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + b"I" * 150 + b"\n")
                i += 1
    asm, alt = bytearray(G.tobytes()), bytearray(H)
    for p in (1000, 7000, 12_345, 22_000, 27_000):
        asm[p] = other_base(asm[p])
    for p in (3000, 12_345, 18_000, 25_000):                  # (12 345 is before the deletion: the same place and the same wrong base in both)
        alt[p] = asm[p] if p == 12_345 else other_base(alt[p])
    asm[5000:5010] = b"N" * 10
    c1, c2 = bytes(asm[:16_000]), bytes(asm[16_000:])
    c2 = c2[:2000] + c2[2000:2600].lower() + c2[2600:]
    for path, contigs in ((d / "asm.fa", [(b"ctg1 hap=1", c1), (b"ctg2", c2)]), (d / "alt.fa", [(b"hapB_1", bytes(alt))])):
        with open(path, "wb") as f:
            for name, s in contigs:
                f.write(b">" + name + b"\n")
                for a in range(0, len(s), 70):
                    f.write(s[a:a + 70] + b"\n")


def qv(x, valid):
    """the value of report.qv_text, or its word"""
    if valid <= 0:
        return "NA"
    if x <= 0:
        return "inf"
    return -10.0 * math.log10(1.0 - (1.0 - x / valid) ** (1.0 / K))


def same_number(got, want, decimals=4):
    """a formatted number within 1e-4 of the value (or the same word)"""
    if isinstance(want, str):
        return got == want
    return re.match(r"^-?\d+\.\d{%d}$" % decimals, got) is not None and abs(float(got) - float("%.*f" % (decimals, want))) <= 1e-4


def expected(d, asm_fa, alt_fa):
    """(P, names / seqs / (counts, runs) of asm and of alt) from the files, through Python dicts"""
    rd = kmer_dict(open(d / "reads.fq", "rb").read().split(b"\n")[1::4], K)
    n1, s1 = read_fasta(d / asm_fa)
    n2, s2 = read_fasta(d / alt_fa)
    d1, d2 = kmer_dict(s1, K), kmer_dict(s2, K)
    return restate_pair(rd, d1, d2), (n1, s1, restate_scan(s1, K, rd, d2, THRE)), (n2, s2, restate_scan(s2, K, rd, d1, THRE))


def check_files(d, P, asm, alt):
    P = [[int(v) for v in row] for row in P]
    # PREFIX.spectra_asm.tsv
    want = "#class\tread_count\tkmers\n" + "".join("%s\t%d\t%d\n" % (CLASSES[j], c, v) for j in range(4) for c, v in enumerate(P[j]) if v)
    assert open(d / "p.spectra_asm.tsv").read() == want
    # PREFIX.diploid.completeness.tsv
    lines = open(d / "p.diploid.completeness.tsv").read().splitlines()
    assert lines[0] == "#set\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tdistinct\tnot_in_reads" and len(lines) == 4
    solid = sum(sum(r[THRE:]) for r in P)
    for ln, (name, js) in zip(lines[1:], (("asm", (1, 3)), ("alt", (2, 3)), ("both", (1, 2, 3)))):
        f = ln.split("\t")
        found = sum(sum(P[j][THRE:]) for j in js)
        assert f[:5] == [name, str(K), str(THRE), str(solid), str(found)], ln
        assert same_number(f[5], 100.0 * found / solid), ln
        assert f[6:] == [str(sum(sum(P[j]) for j in js)), str(sum(P[j][0] for j in js))], ln
    # PREFIX.diploid.tsv
    lines = open(d / "p.diploid.tsv").read().splitlines()
    assert lines[0] == ("#set\tcontig\tlength\twindows\tvalid\tunreliable\tabsent\tQV_unreliable\tQV_absent\tprivate_solid\tprivate_weak\tshared_unreliable"
                        "\tprivate_fraction")
    rows, stars = [], []
    for which, (names, seqs, (counts, _)) in (("asm", asm), ("alt", alt)):
        rows += [(which, n, len(s), c) for n, s, c in zip(names, seqs, counts)]
        stars.append((which, "*", sum(len(s) for s in seqs), tuple(sum(c[i] for c in counts) for i in range(6))))
        rows.append(stars[-1])
    rows.append(("both", "*", stars[0][2] + stars[1][2], tuple(a + b for a, b in zip(stars[0][3], stars[1][3]))))
    assert len(lines) == 1 + len(rows)
    for ln, (which, name, length, c) in zip(lines[1:], rows):
        f = ln.split("\t")
        w, v, u, a, ps, pw = c
        assert f[:7] == [which, name, str(length), str(w), str(v), str(u), str(a)], ln
        assert same_number(f[7], qv(u, v)) and same_number(f[8], qv(a, v)), ln
        assert f[9:12] == [str(ps), str(pw), str(u - pw)], ln
        assert same_number(f[12], (ps + pw) / v if v else "NA"), ln
    # PREFIX.private.{asm,alt}.bed
    for which, (names, _, (_, runs)) in (("asm", asm), ("alt", alt)):
        lines = open(d / ("p.private.%s.bed" % which)).read().splitlines()
        assert len(lines) == len(runs), which
        for ln, (seq, start, nk, kind, sr) in zip(lines, runs):
            f = ln.split("\t")
            assert f[:5] == [names[seq], str(start), str(start + nk + K - 1), {1: "solid", 2: "weak"}[kind], str(nk)], ln
            assert same_number(f[5], sr / nk, 2), ln


def prefix_files(d):
    return sorted(fn for fn in os.listdir(d) if fn.startswith("p."))


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("diploid")
    write_inputs(d)
    out = {"dir": d}
    base = ["-r", "reads.fq", "-k", str(K), "--threshold", str(THRE), "--spectra"]
    for mode, flags in (("plain", ["-a", "asm.fa"]), ("alt", ["-a", "asm.fa", "--alt", "alt.fa"]), ("swapped", ["-a", "alt.fa", "--alt", "asm.fa"])):
        os.mkdir(d / mode)
        out[mode] = cli(d, flags + base + ["-o", "%s/p" % mode], env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.kmerqc")
    return out


def test_without_alt_the_evaluator_writes_what_it_always_wrote(runs):
    d = runs["dir"]
    assert prefix_files(d / "plain") == PLAIN_FILES
    assert not [m for m in messages(runs["plain"].stdout) if "iploid" in m] and "[diploid]" not in runs["plain"].stderr


def test_with_alt_five_more_files_and_every_other_file_unchanged(runs):
    d = runs["dir"]
    assert prefix_files(d / "alt") == sorted(PLAIN_FILES + NEW_FILES)
    for fn in PLAIN_FILES:
        assert open(d / "alt" / fn, "rb").read() == open(d / "plain" / fn, "rb").read(), fn
    m0, m1 = messages(runs["plain"].stdout), messages(runs["alt"].stdout)
    same = [m.replace("alt/p.", "plain/p.") for m in m1[:len(m0)]]          # (a log line names its file with the run's prefix)
    assert same == m0 and len(m1) == len(m0) + 3, "the three log lines come after the existing ones"
    assert m1[-3].startswith("Diploid k-mer completeness: asm ") and m1[-2].startswith("Diploid dense k-mer QV (unreliable k-mers): asm ")
    assert m1[-1].startswith("Diploid private windows: asm ") and m1[-1].endswith(" in alt/p.private.asm.bed and alt/p.private.alt.bed")
    assert re.search(r"^\[diploid\] device seconds: join \d+\.\d{6} scan asm \d+\.\d{6} scan alt \d+\.\d{6}$", runs["alt"].stderr, re.M)


def test_the_new_files_equal_the_restatement(runs):
    d = runs["dir"]
    P, asm, alt = expected(d, "asm.fa", "alt.fa")
    assert asm[0] == ["ctg1", "ctg2"] and alt[0] == ["hapB_1"]
    for _, _, (counts, runs_) in (asm, alt):                              # the case is worth running: both classes on both haplotypes
        assert sum(c[4] for c in counts) > 500 and sum(c[5] for c in counts) >= 3 * K and {r[3] for r in runs_} == {1, 2}
        assert sum(c[2] - c[5] for c in counts) >= K, "unreliable windows both haplotypes hold"
    assert all(int(P[j].sum()) > 0 for j in range(4)) and int(P[1][0]) > 0 and int(P[2][0]) > 0 and int(P[3][0]) > 0
    check_files(d / "alt", P, asm, alt)
    # the log lines carry the files' numbers
    m = messages(runs["alt"].stdout)
    comp = [ln.split("\t") for ln in open(d / "alt" / "p.diploid.completeness.tsv").read().splitlines()[1:]]
    assert m[-3] == "Diploid k-mer completeness: asm %s %%, alt %s %%, both %s %% (%s of %s solid k-mers, threshold %d)" % (
        comp[0][5], comp[1][5], comp[2][5], comp[2][4], comp[2][3], THRE)
    star = {f[0]: f for f in (ln.split("\t") for ln in open(d / "alt" / "p.diploid.tsv").read().splitlines()[1:]) if f[1] == "*"}
    assert m[-2] == "Diploid dense k-mer QV (unreliable k-mers): asm %s, alt %s, both %s" % (star["asm"][7], star["alt"][7], star["both"][7])
    assert m[-1].startswith("Diploid private windows: asm %s solid %s weak in %d runs; alt %s solid %s weak in %d runs in " % (
        star["asm"][9], star["asm"][10], len(asm[2][1]), star["alt"][9], star["alt"][10], len(alt[2][1])))


def test_the_asm_rows_repeat_the_spectrum_and_the_report(runs):
    d = runs["dir"] / "alt"
    comp = open(d / "p.completeness.tsv").read().splitlines()[1].split("\t")
    mine = open(d / "p.diploid.completeness.tsv").read().splitlines()[1].split("\t")
    assert comp[0] == "asm" and mine[0] == "asm" and mine[3:] == comp[3:], "solid, found, completeness, distinct, not in the reads"
    rep = [ln.split("\t") for ln in open(d / "p.kmer_qv.tsv").read().splitlines()[1:]]
    dip = [f for f in (ln.split("\t") for ln in open(d / "p.diploid.tsv").read().splitlines()[1:]) if f[0] == "asm"]
    assert len(rep) == len(dip) == 3
    for r, m in zip(rep, dip):
        assert r[0] == m[1] and r[2:9] == m[2:9]


def test_swapping_the_haplotypes_swaps_rows_and_classes(runs):
    d = runs["dir"]
    a, s = d / "alt", d / "swapped"
    assert prefix_files(s) == sorted(PLAIN_FILES + NEW_FILES)
    assert open(s / "p.private.asm.bed", "rb").read() == open(a / "p.private.alt.bed", "rb").read()
    assert open(s / "p.private.alt.bed", "rb").read() == open(a / "p.private.asm.bed", "rb").read()
    swap = {"asm": "alt", "alt": "asm", "both": "both", "asm_only": "alt_only", "alt_only": "asm_only", "reads_only": "reads_only", "shared": "shared"}

    def swapped_lines(path):
        lines = open(path).read().splitlines()
        return lines[0], sorted("\t".join([swap[ln.split("\t")[0]]] + ln.split("\t")[1:]) for ln in lines[1:])
    for fn in ("p.spectra_asm.tsv", "p.diploid.completeness.tsv", "p.diploid.tsv"):
        head, body = swapped_lines(s / fn)
        lines = open(a / fn).read().splitlines()
        assert head == lines[0] and body == sorted(lines[1:]), fn
    check_files(s, *expected(d, "alt.fa", "asm.fa"))                     # (and in the order the format asks for)
