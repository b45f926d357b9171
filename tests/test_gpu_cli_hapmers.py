"""GPU: `python -m jasper_amd.kmerqc ... --hapmers` and `python -m jasper_amd.cli ... --hapmers` on a tiny synthetic trio.

Without the flag nothing changes; with it the new files equal, byte for byte, what this file computes with Python dicts from the three
read files, asm.fa and the polished FASTA it reads back: its own restatement of the scan and the census (include/jasper_hip.h), of the
threshold rule, of the phase-block rule and of the file formats (README.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cli_spectra import COMMON, ROOT, cli, messages, read_fasta

pytestmark = pytest.mark.gpu
K = 25
MAT, PAT = 1, 2
_RC = bytes.maketrans(b"ACGT", b"TGCA")
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
PARENTS = ["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq"]
HAPMER_FILES = ("asm.fa.hapmer_completeness.tsv", "asm.fa.hapmers.after.bed", "asm.fa.hapmers.before.bed", "asm.fa.hapmers.tsv",
                "asm.fa.phased_blocks.after.bed", "asm.fa.phased_blocks.before.bed")
SHORT_RANGE, MAX_SWITCHES = 20000, 100
HAP = {MAT: "mat", PAT: "pat"}


def write_inputs(d):
    """a 6 kb genome; the mother's and the father's haplotype carry independent SNPs about every 250 bases; the child has both.  ctg1 is
    the maternal haplotype with a paternal stretch in it (a switch) and three wrong bases for the polisher, ctg2 the paternal one, ctg3
    is shorter than k.  Reads: 150 bases, 0.3 % errors, the child at 30x per haplotype, each parent at 40x."""
    from jasper_amd import synth
    rng = np.random.default_rng(515)
    genome = synth.make_genome(rng, 6000)
    haps = []
    for _ in range(2):
        h = genome.copy()
        pos = rng.choice(len(h), len(h) // 250, replace=False)
        h[pos] = synth.ACGT[(np.searchsorted(synth.ACGT, h[pos]) + rng.integers(1, 4, len(pos))) % 4]
        haps.append(h)
    mh, ph = haps

    def fastq(path, parts):
        with open(path, "wb") as f:
            for g, cov in parts:
                for i, r in enumerate(synth.make_reads_stream(rng, g, cov, 150, 0.003).reshape(-1, 151)[:, :150]):
                    f.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + b"I" * 150 + b"\n")
    fastq(d / "reads.fq", [(mh, 30), (ph, 30)])
    fastq(d / "mat.fq", [(mh, 40)])
    fastq(d / "pat.fq", [(ph, 40)])
    c1 = np.concatenate([mh[:1500], ph[1500:1900], mh[1900:3500]])
    for p in (300, 1000, 2900):
        c1[p] = synth.ACGT[(np.searchsorted(synth.ACGT, c1[p]) + 1) % 4]
    c2 = ph[3400:6000].copy()
    c2[700:760] = np.frombuffer(c2[700:760].tobytes().lower(), dtype=np.uint8)
    with open(d / "asm.fa", "wb") as f:
        for name, s in ((b"ctg1 child=1", c1.tobytes()), (b"ctg2", c2.tobytes()), (b"ctg3", mh[:K - 1].tobytes())):
            f.write(b">" + name + b"\n")
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + b"\n")


def window_kmers(seq):
    """per window of one sequence: its canonical k-mer, or None where one of its K bytes is no base (case folded)"""
    b = (seq.encode() if isinstance(seq, str) else bytes(seq)).upper()
    out = []
    for i in range(len(b) - K + 1):
        w = b[i:i + K]
        out.append(None if w.strip(b"ACGT") else min(w, w.translate(_RC)[::-1]))
    return out


def kmer_dict(seqs):
    d = {}
    for s in seqs:
        for key in window_kmers(s):
            if key is not None:
                d[key] = d.get(key, 0) + 1
    return d


def reads_dict(path):
    return kmer_dict(open(path, "rb").read().split(b"\n")[1::4])


def scan(seqs, md, pd, rd, tm, tp, tc):
    """the hap-mer scan of include/jasper_hip.h: per sequence (windows, valid, mat, pat), and the maximal runs (seq, start, n, kind)"""
    counts, runs = [], []
    for si, s in enumerate(seqs):
        cls = []
        for key in window_kmers(s):
            if key is None:
                cls.append(-1)
            elif rd.get(key, 0) < tc:
                cls.append(0)
            else:
                m, p = md.get(key, 0), pd.get(key, 0)
                cls.append(MAT if m >= tm and p == 0 else PAT if p >= tp and m == 0 else 0)
        counts.append((len(cls), sum(c >= 0 for c in cls), cls.count(MAT), cls.count(PAT)))
        i = 0
        while i < len(cls):
            j = i
            while j < len(cls) and cls[j] == cls[i]:
                j += 1
            if cls[i] > 0:
                runs.append((si, i, j - i, cls[i]))
            i = j
    return counts, runs


def threshold_rule(d):
    """the histogram followed downhill from its first row; the first row that rises ends the descent; half the multiplicity of the
    descent's last row"""
    h = {}
    for c in d.values():
        h[min(c, 10001)] = h.get(min(c, 10001), 0) + 1
    rows = sorted(h.items())
    floor_n, half = rows[0][1], 0
    for m, n in rows[1:]:
        if n > floor_n:
            return half
        floor_n, half = n, m // 2
    return None


def phase_blocks(markers, short_range=SHORT_RANGE, max_switches=MAX_SWITCHES):
    """the block rule of the issue, on one contig's (start, n, kind): -> [(start, end, kind, markers, kmers, switch_markers, switch_kmers)]"""
    out, blk, pend = [], None, []

    def start(ms):
        return {"own": list(ms), "sm": 0, "sk": 0}

    def emit(b):
        own = b["own"]
        out.append((own[0][0], own[-1][0] + own[-1][1] + K - 1, own[0][2], len(own), sum(m[1] for m in own), b["sm"], b["sk"]))

    for m in markers:
        if blk is None:
            blk = start([m])
        elif m[2] == blk["own"][0][2]:
            blk["sm"] += len(pend)
            blk["sk"] += sum(p[1] for p in pend)
            pend = []
            blk["own"].append(m)
        else:
            pend.append(m)
            if len(pend) > max_switches or m[0] + m[1] - pend[0][0] > short_range:
                emit(blk)
                blk, pend = start(pend), []
    if blk is not None:
        emit(blk)
    if pend:
        emit(start(pend))
    return out


def n50(blocks):
    lens = sorted((b[1] - b[0] for b in blocks), reverse=True)
    acc = 0
    for ln in lens:
        acc += ln
        if 2 * acc >= sum(lens):
            return ln
    return 0


def rate(n_markers, blocks):
    own, sk = sum(b[4] for b in blocks), sum(b[6] for b in blocks)
    return "NA" if n_markers == 0 else "%.4f" % (100.0 * sk / (own + sk))


class Truth:
    """everything the files of one stage hold, from dicts"""

    def __init__(self, names, seqs, md, pd, rd, tm, tp, tc, short_range=SHORT_RANGE, max_switches=MAX_SWITCHES):
        self.names, self.seqs = names, seqs
        self.counts, self.runs = scan(seqs, md, pd, rd, tm, tp, tc)
        self.markers = [[(r[1], r[2], r[3]) for r in self.runs if r[0] == i] for i in range(len(seqs))]
        self.blocks = [phase_blocks(m, short_range, max_switches) for m in self.markers]
        ad = kmer_dict(seqs)
        self.census = []
        for own, other, thre in ((md, pd, tm), (pd, md, tp)):
            H = [x for x, c in own.items() if c >= thre and other.get(x, 0) == 0 and rd.get(x, 0) >= tc]
            self.census.append((len(H), sum(1 for x in H if ad.get(x, 0) >= 1), sum(ad.get(x, 0) for x in H)))

    def row(self, name, stage, i):
        """i: contig index, None = the contig is missing, "*" = all"""
        if i is None:
            return "%s\t%s\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tNA\n" % (name, stage)
        idx = range(len(self.seqs)) if i == "*" else [i]
        c = [sum(self.counts[j][f] for j in idx) for f in range(4)]
        ms, bs = [m for j in idx for m in self.markers[j]], [b for j in idx for b in self.blocks[j]]
        return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, stage, sum(len(self.seqs[j]) for j in idx), c[0], c[1], c[2], c[3], len(ms), len(bs), n50(bs),
                                                                      sum(b[5] for b in bs), sum(b[6] for b in bs), rate(len(ms), bs))

    def bed(self):
        return "".join("%s\t%d\t%d\t%s\t%d\n" % (self.names[s], a, a + n + K - 1, HAP[kind], n) for s, a, n, kind in self.runs)

    def blocks_bed(self):
        return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % ((name, b[0], b[1], HAP[b[2]]) + b[3:]) for name, bs in zip(self.names, self.blocks) for b in bs)

    def completeness_rows(self, stage, tm, tp, tc):
        return "".join("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (stage, hap, K, thre, tc, h, f, "NA" if h == 0 else "%.4f" % (100.0 * f / h), occ)
                       for hap, thre, (h, f, occ) in (("mat", tm, self.census[0]), ("pat", tp, self.census[1])))

    def log(self):
        bs = [b for x in self.blocks for b in x]
        comp = ["NA" if h == 0 else "%.4f" % (100.0 * f / h) for h, f, _ in self.census]
        return "%d mat and %d pat windows in %d markers, %d blocks (N50 %d), switch rate %s; hap-mer completeness mat %s pat %s" % (
            sum(c[2] for c in self.counts), sum(c[3] for c in self.counts), len(self.runs), len(bs), n50(bs), rate(len(self.runs), bs), comp[0], comp[1])


TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\tmat\tpat\tmarkers\tblocks\tblock_n50\tswitch_markers\tswitch_kmers\tswitch_rate\n"
COMPLETENESS_HEADER = "#stage\thap\tk\tparent_threshold\tchild_threshold\thapmers\tfound\tcompleteness\toccurrences\n"


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("hapmers", PARENTS)):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d1 = runs["hapmers"][0]
    md, pd, rd = reads_dict(d1 / "mat.fq"), reads_dict(d1 / "pat.fq"), reads_dict(d1 / "reads.fq")
    tm, tp, tc = threshold_rule(md), threshold_rule(pd), threshold_rule(rd)
    assert tm >= 2 and tp >= 2 and tc >= 2 and tc == int(open(d1 / "threshold.txt").read().split()[0])
    names, seqs = read_fasta(d1 / "asm.fa")
    pnames, pseqs = read_fasta(d1 / "asm.fa.polished.fasta")
    assert names == ["ctg1", "ctg2", "ctg3"] and pnames == names and pseqs != seqs
    return dict(md=md, pd=pd, rd=rd, tm=tm, tp=tp, tc=tc, names=names, before=Truth(names, seqs, md, pd, rd, tm, tp, tc), after=Truth(names, pseqs, md, pd, rd, tm, tp, tc))


def test_driver_hapmer_files_and_nothing_else_changes(runs, truth):
    (d0, p0), (d1, p1) = runs["plain"], runs["hapmers"]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    for fn in COMMON:
        assert os.path.isfile(d0 / fn), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if "Hap-mer scan" in m]
    assert len(extra) == 1 and [m for m in m1 if m not in extra] == m0
    assert m1.index(extra[0]) == len(m1) - 2 and "Polished sequence is in" in m1[-1]
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(HAPMER_FILES)
    assert not [fn for fn in os.listdir(d0) if "hapmer" in fn or "phased" in fn]
    t, b, a = truth, truth["before"], truth["after"]
    names = t["names"]
    want = TSV_HEADER + "".join(b.row(n, "before", i) + a.row(n, "after", i) for i, n in enumerate(names)) + b.row("*", "before", "*") + a.row("*", "after", "*")
    assert open(d1 / "asm.fa.hapmers.tsv").read() == want
    assert open(d1 / "asm.fa.hapmers.before.bed").read() == b.bed()
    assert open(d1 / "asm.fa.hapmers.after.bed").read() == a.bed()
    assert open(d1 / "asm.fa.phased_blocks.before.bed").read() == b.blocks_bed()
    assert open(d1 / "asm.fa.phased_blocks.after.bed").read() == a.blocks_bed()
    tm, tp, tc = t["tm"], t["tp"], t["tc"]
    assert open(d1 / "asm.fa.hapmer_completeness.tsv").read() == COMPLETENESS_HEADER + b.completeness_rows("before", tm, tp, tc) + a.completeness_rows("after", tm, tp, tc)
    assert extra[0] == "Hap-mer scan (thresholds mat %d pat %d child %d): before polishing %s; after polishing %s" % (tm, tp, tc, b.log(), a.log())
    # the workload holds what the scan is for: both kinds of marker, the paternal stretch inside ctg1 as switches of one maternal block,
    # ctg2 one paternal block, the scan's totals equal to the census's occurrences (the assembly's table is counted from these contigs)
    kinds1 = [m[2] for m in b.markers[0]]
    assert kinds1.count(MAT) >= 5 and kinds1.count(PAT) >= 1 and len(b.blocks[0]) == 1 and b.blocks[0][0][2] == MAT and b.blocks[0][0][5] >= 1
    assert [x[2] for x in b.blocks[1]] == [PAT] and b.markers[2] == [] and b.counts[2] == (0, 0, 0, 0)
    assert b.census[0][2] == sum(c[2] for c in b.counts) and b.census[1][2] == sum(c[3] for c in b.counts)
    assert 0 < b.census[0][1] < b.census[0][0]


def test_kmerqc_hapmers_from_read_files_and_from_databases(KT, runs, truth, tmp_path):
    d1 = runs["hapmers"][0]
    t, b = truth, truth["before"]
    names, tm, tp, tc = t["names"], t["tm"], t["tp"], t["tc"]
    seen = set(os.listdir(d1))
    want = {"hapmers.tsv": TSV_HEADER + "".join(b.row(n, "asm", i) for i, n in enumerate(names)) + b.row("*", "asm", "*"),
            "hapmers.bed": b.bed(), "phased_blocks.bed": b.blocks_bed(),
            "hapmer_completeness.tsv": COMPLETENESS_HEADER + b.completeness_rows("asm", tm, tp, tc)}
    p = cli(d1, ["-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "-o", str(tmp_path / "qr")] + PARENTS, module="jasper_amd.kmerqc")
    assert set(os.listdir(d1)) == seen
    assert sorted(os.listdir(tmp_path)) == sorted(["qr." + fn for fn in want] + ["qr.kmer_qv.tsv", "qr.unreliable.bed"])
    for fn, text in want.items():
        assert open(tmp_path / ("qr." + fn)).read() == text, fn
    lines = [m for m in messages(p.stdout) if "Hap-mer scan" in m]
    assert lines == ["Hap-mer scan (thresholds mat %d pat %d child %d): %s in %s.hapmers.bed" % (tm, tp, tc, b.log(), tmp_path / "qr")]
    # the parents as databases written by the project's own writer, the child's from the driver's run; --spectra and --copies beside it
    for who in ("mat", "pat"):
        tab = KT(K, min_slots=1 << 20)
        tab.count_files([str(d1 / (who + ".fq"))])
        tab.write_jf(str(tmp_path / (who + ".jf")))
        tab.close()
    cli(d1, ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "-o", str(tmp_path / "qj"), "--hapmers", "--mat-jf", str(tmp_path / "mat.jf"), "--pat-jf", str(tmp_path / "pat.jf"),
             "--spectra", "--copies"], module="jasper_amd.kmerqc")
    for fn, text in want.items():
        assert open(tmp_path / ("qj." + fn)).read() == text, fn
    plain = tmp_path / "plain"
    cli(d1, ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "-o", str(plain), "--spectra", "--copies"], module="jasper_amd.kmerqc")
    for ext in ("kmer_qv.tsv", "unreliable.bed", "spectra_cn.tsv", "completeness.tsv", "copies.tsv", "copies.bed"):
        assert open("%s.%s" % (plain, ext), "rb").read() == open(tmp_path / ("qj." + ext), "rb").read(), ext
    # given thresholds and block parameters: the files of the dicts for those
    cli(d1, ["-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "-o", str(tmp_path / "qt"), "--threshold", "3", "--mat-threshold", "1", "--pat-threshold", str(tp + 5),
             "--phase-short-range", "300", "--phase-max-switches", "1"] + PARENTS, module="jasper_amd.kmerqc")
    g = Truth(names, b.seqs, t["md"], t["pd"], t["rd"], 1, tp + 5, 3, 300, 1)
    assert len(g.blocks[0]) > len(b.blocks[0])
    assert open(tmp_path / "qt.hapmers.tsv").read() == TSV_HEADER + "".join(g.row(n, "asm", i) for i, n in enumerate(names)) + g.row("*", "asm", "*")
    assert open(tmp_path / "qt.phased_blocks.bed").read() == g.blocks_bed()
    assert open(tmp_path / "qt.hapmer_completeness.tsv").read() == COMPLETENESS_HEADER + g.completeness_rows("asm", 1, tp + 5, 3)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


def test_bad_flags_end_the_driver_before_it_starts(runs, tmp_path):
    for bad, message in ((["--mat", "mat.fq"], "give --hapmers as well"), (["--hapmers", "--mat", "mat.fq"], "needs both parents"),
                         (PARENTS + ["--mat-threshold", "0"], "integers of at least 1")):
        d = runs["plain"][0]
        before = set(os.listdir(d))
        p = subprocess.run([sys.executable, "-m", "jasper_amd.cli"] + ARGS + bad, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1 and message in p.stderr and set(os.listdir(d)) == before
