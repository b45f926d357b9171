"""GPU: `python -m jasper_amd.cli ... --gaps [--gaps-fill]` and `python -m jasper_amd.kmerqc ... --gaps --gap-long-runs` on a small
assembly with two planted gaps, one of them with a dirty edge, and reads with errors at 60x.  As for diploid_k25 in
test_gpu_cli_compound.py a threshold.txt is written beforehand: the driver, as src/jasper.sh:195-206, uses the one it finds when the
histogram gives none.

With the flags the gap files and the new log line equal jasper_amd/gaps.py's texts (checked on hand-made sites and records in
test_gaps_host.py) of what the restatement of test_gaps_host.py lists over a Python dict of the reads' k-mers; the filled FASTA differs
from the polished one at the two sites only; with --report as well the report files are those of --report alone."""
import os

import numpy as np
import pytest

from test_gaps_host import restate_gaps
from test_gpu_cli_spectra import REPORT_FILES, cli, messages, read_fasta
from test_gpu_copies import dict_counter, kmer_dict

pytestmark = pytest.mark.gpu
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
GAP_FILES = ("asm.fa.gapfills.after.tsv", "asm.fa.gapfills.before.tsv", "asm.fa.gaps.after.bed", "asm.fa.gaps.before.bed", "asm.fa.gaps.tsv")
GAPS = ((3000, 140, 100), (8000, 37, 60))             # (where, bases taken out, Ns put in)


def make_inputs(seed=52):
    """(reads [bytes], contigs [bytes]): a genome of 12 000 bases, 60x of reads of 150 with 0.3 % errors, and an assembly of two contigs:
    the first holds two gaps -- 140 bases behind 100 Ns, and 37 bases behind 60 Ns with a wrong base 5 bases before the Ns -- and a few
    wrong bases elsewhere for the polisher; the second is clean"""
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, 12_000)
    reads = synth.make_reads_stream(rng, genome, 60, 150, 0.003).reshape(-1, 151)[:, :150]
    g = bytearray(genome.tobytes())
    for p in (1000, 5000, 9500, 8000 - 5):
        g[p] = b"ACGT"[(b"ACGT".index(g[p]) + 1) & 3]
    c1 = bytes(g[:10_000])
    for at, took, ns in sorted(GAPS, reverse=True):
        c1 = c1[:at] + b"N" * ns + c1[at + took:]
    return [r.tobytes() for r in reads], [c1, bytes(g[10_000:])], genome.tobytes()


def write_inputs(d):
    reads, contigs, _ = make_inputs()
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    with open(d / "asm.fa", "wb") as f:
        for i, s in enumerate(contigs):
            f.write(b">ctg%d planted\n" % (i + 1))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + b"\n")
    with open(d / "threshold.txt", "w") as f:          # the histogram of so small a read set may have no usable minimum: then the driver keeps this one
        f.write("10\n")


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("gaps", ["--gaps", "--gaps-fill"]), ("report", ["--report"]), ("both", ["--report", "--gaps"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d = runs["gaps"][0]
    thre = int(open(d / "threshold.txt").read().split()[0])
    reads, contigs, genome = make_inputs()
    count = dict_counter(kmer_dict(reads, K))
    names, seqs = read_fasta(d / "asm.fa")
    pnames, pseqs = read_fasta(d / "asm.fa.polished.fasta")
    assert pnames == names and thre >= 1 and [s.encode() for s in seqs] == contigs
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, genome=genome, count=count,
                before=restate_gaps(seqs, K, count, thre, 1000, K, False), after=restate_gaps(pseqs, K, count, thre, 1000, K, False))


def test_gap_files_fill_and_log_line(runs, truth):
    from jasper_amd import gaps, repair
    d, p = runs["gaps"]
    t = truth
    (c0, s0, r0), (c1, s1, r1) = t["before"], t["after"]
    assert c0[0][:5] == (2, 2, 2, 2, 2) and c1[0][:5] == (2, 2, 2, 2, 2) and s0[1][7] == 5      # both gaps close, in either stage; the dirty edge is 5 bases
    len0, len1 = [len(s) for s in t["seqs"]], [len(s) for s in t["pseqs"]]
    assert open(d / "asm.fa.gaps.tsv").read() == gaps.gaps_tsv_text(t["names"], [("before", len0, c0), ("after", len1, c1)])
    for stage, sites, recs in (("before", s0, r0), ("after", s1, r1)):
        assert open(d / ("asm.fa.gaps.%s.bed" % stage)).read() == gaps.bed_text(t["names"], sites, recs)
        assert open(d / ("asm.fa.gapfills.%s.tsv" % stage)).read() == gaps.fills_tsv_text(t["names"], recs)
    assert not [fn for fn in os.listdir(d) if fn.endswith(".tmp")] and set(GAP_FILES) | {"asm.fa.gapfilled.fasta"} <= set(os.listdir(d))
    assert [m for m in messages(p.stdout) if m.startswith("Gap scan")] == [gaps.log_text(c0, c1)]
    # the filled FASTA: the polished one with the two sites replaced, and what it holds there is the genome
    polished_text = open(d / "asm.fa.polished.fasta", newline="").read()
    filled = gaps.fill_sequences(t["pseqs"], s1, r1)
    assert open(d / "asm.fa.gapfilled.fasta", newline="").read() == repair.fasta_text(polished_text, filled)
    fnames, fseqs = read_fasta(d / "asm.fa.gapfilled.fasta")
    assert fnames == t["names"] and fseqs[1] == t["pseqs"][1] and "N" not in fseqs[0]
    (_, a0, q0, *_), (_, a1, q1, *_) = s1
    assert fseqs[0][:a0] == t["pseqs"][0][:a0] and fseqs[0][len(fseqs[0]) - (len1[0] - q1):] == t["pseqs"][0][q1:]
    assert fseqs[0][a0 + r1[0][3]:a1 - (q0 - a0) + r1[0][3]] == t["pseqs"][0][q0:a1]
    assert fseqs[0][2900:3300].encode() == t["genome"][2900:3300] and len(fseqs[0]) == len1[0] - (q0 - a0) - (q1 - a1) + r1[0][3] + r1[1][3]


def test_with_report_the_report_files_are_those_of_report_alone(runs):
    (dr, pr), (db, pb), (dg, _) = runs["report"], runs["both"], runs["gaps"]
    assert sorted(set(os.listdir(db)) - set(os.listdir(dr))) == sorted(GAP_FILES)
    for fn in REPORT_FILES:
        assert open(db / fn, "rb").read() == open(dr / fn, "rb").read(), fn
    for fn in GAP_FILES:
        assert open(db / fn, "rb").read() == open(dg / fn, "rb").read(), fn
    mr, mb = messages(pr.stdout), messages(pb.stdout)
    assert [m for m in mb if not m.startswith("Gap scan")] == mr and len(mb) == len(mr) + 1


def test_kmerqc_with_the_flags(runs, truth, tmp_path):
    from jasper_amd import gaps
    d = runs["gaps"][0]
    t = truth
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(t["thre"])]
    p = cli(d, base + ["-o", str(tmp_path / "qc"), "--gaps", "--gap-long-runs", "--gap-max-len", "300"], module="jasper_amd.kmerqc")
    c0, s0, r0 = restate_gaps(t["seqs"], K, t["count"], t["thre"], 300, K, True)
    len0 = [len(s) for s in t["seqs"]]
    assert open(tmp_path / "qc.gaps.tsv").read() == gaps.gaps_tsv_text(t["names"], [("asm", len0, c0)])
    assert open(tmp_path / "qc.gaps.bed").read() == gaps.bed_text(t["names"], s0, r0)
    assert open(tmp_path / "qc.gapfills.tsv").read() == gaps.fills_tsv_text(t["names"], r0)
    assert [m for m in messages(p.stdout) if m.startswith("Gap scan")] == ["Gap scan: %s in %s.gaps.bed" % (gaps.stage_log_text(c0), tmp_path / "qc")]
    # without the flags: the same report files, no gap file, no such line
    p0 = cli(d, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    for ext in (".kmer_qv.tsv", ".unreliable.bed"):
        assert open(str(tmp_path / "q0") + ext, "rb").read() == open(str(tmp_path / "qc") + ext, "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["q0.kmer_qv.tsv", "q0.unreliable.bed", "qc.gapfills.tsv", "qc.gaps.bed", "qc.gaps.tsv", "qc.kmer_qv.tsv", "qc.unreliable.bed"]
    assert [m for m in messages(p.stdout) if not m.startswith("Gap scan")] == [m.replace(str(tmp_path / "q0"), str(tmp_path / "qc")) for m in messages(p0.stdout)]
