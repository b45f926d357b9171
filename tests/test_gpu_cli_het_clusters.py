"""GPU: `python -m jasper_amd.cli ... --indels --het-clusters` and `python -m jasper_amd.kmerqc ... --indels --het-clusters` on a small
planted diploid input: two haplotypes that differ by clusters of differences less than k apart -- pairs and triples of SNPs, a SNP beside
an insertion or a deletion -- reads of both, and the first haplotype as the assembly.

With the flag the three het-cluster files and the new log line equal jasper_amd/hetclusters.py's texts (checked on hand-made records in
test_het_clusters_host.py) of what the restatement of test_het_clusters_host.py lists over a Python dict of the reads' k-mers; every
other file is byte for byte that of the same run without the flag; with the other extensions as well their files are their own."""
import os

import numpy as np
import pytest

from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_copies import dict_counter, kmer_dict
from test_het_clusters_host import restate_clusters, substitute
from test_indels_host import rand_bases
from test_indels_mixed_host import plant_strings

pytestmark = pytest.mark.gpu
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2", "--indels"]
CLUSTER_FILES = ("asm.fa.het_clusters.after.vcf", "asm.fa.het_clusters.before.vcf", "asm.fa.het_clusters.tsv")


def write_inputs(d):
    """two contigs of one haplotype as the assembly (a stretch of the second in lower case); the other haplotype has a cluster every
    500 bases; 150-base reads of both at 25x each"""
    from jasper_amd import synth
    rng = np.random.default_rng(79)
    h1 = synth.make_genome(rng, 16_000).tobytes()
    at, ev = [], []
    for i, p in enumerate(range(400, 15_600, 500)):
        dist = (1, 4, 24, 12, 7, 2, 20, 9)[i % 8]
        at += [p, p + dist] + ([p + dist // 2] if i % 4 == 3 else [])
        if i % 5 == 1:
            ev.append((p + dist + 3, "del", 1 + i % 3))
        if i % 5 == 2:
            ev.append((p + dist + 4, "ins", rand_bases(rng, 1 + i % 4)))
    h2 = plant_strings(substitute(h1, at), ev)
    with open(d / "reads.fq", "wb") as f:
        n = 0
        for h in (h1, h2):
            reads = synth.make_reads_stream(rng, np.frombuffer(h, dtype=np.uint8), 25, 150, 0.002).reshape(-1, 151)[:, :150]
            for r in reads:
                f.write(b"@r%d\n" % n + r.tobytes() + b"\n+\n" + b"I" * 150 + b"\n")
                n += 1
    with open(d / "asm.fa", "wb") as f:
        for i, s in enumerate((h1[:9000], h1[9000:9400] + h1[9400:11_000].lower() + h1[11_000:])):
            f.write(b">ctg%d sample=%d\n" % (i + 1, i))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + b"\n")


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("indels", []), ("clusters", ["--het-clusters"]), ("others", ["--variants", "--indel-mixed"]),
                        ("all", ["--variants", "--indel-mixed", "--het-clusters", "--het-cluster-max-len", "13"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d = runs["clusters"][0]
    thre = int(open(d / "threshold.txt").read().split()[0])
    count = dict_counter(kmer_dict(open(d / "reads.fq", "rb").read().split(b"\n")[1::4], K))
    names, seqs = read_fasta(d / "asm.fa")
    pnames, pseqs = read_fasta(d / "asm.fa.polished.fasta")
    assert pnames == names and thre >= 1
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, count=count, before=restate_clusters(seqs, K, count, thre, 64),
                after=restate_clusters(pseqs, K, count, thre, 64))


def test_cluster_files_and_log_line(runs, truth):
    from jasper_amd import hetclusters
    (d0, p0), (d1, p1) = runs["indels"], runs["clusters"]
    t = truth
    (c0, r0), (c1, r1) = t["before"], t["after"]
    # the input holds what the flag is for, on both contigs, under lower case, of both types
    assert len(r0) >= 20 and {r[0] for r in r0} == {0, 1} and any(r[2] != r[3] for r in r0) and any(r[2] == r[3] for r in r0)
    assert any(t["seqs"][r[0]][r[1]].islower() for r in r0)
    len0, len1 = [len(s) for s in t["seqs"]], [len(s) for s in t["pseqs"]]
    assert open(d1 / "asm.fa.het_clusters.tsv").read() == hetclusters.het_clusters_tsv_text(t["names"], [("before", len0, c0), ("after", len1, c1)])
    assert open(d1 / "asm.fa.het_clusters.before.vcf").read() == hetclusters.vcf_text(K, t["thre"], 64, t["names"], len0, t["seqs"], r0)
    assert open(d1 / "asm.fa.het_clusters.after.vcf").read() == hetclusters.vcf_text(K, t["thre"], 64, t["names"], len1, t["pseqs"], r1)
    # without the flag: the same files but the three, byte for byte, and the same log lines but one, right after the indel scan's
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(CLUSTER_FILES) and set(os.listdir(d0)) <= set(os.listdir(d1))
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if m.startswith("Het clusters")]
    assert extra == [hetclusters.log_text(c0, c1)] and [m for m in m1 if m not in extra] == m0
    assert m1[m1.index(extra[0]) - 1].startswith("Indel scan:")


def test_with_the_other_extensions_every_file_is_its_own(runs, truth):
    from jasper_amd import hetclusters
    (do, po), (da, pa) = runs["others"], runs["all"]
    t = truth
    assert sorted(set(os.listdir(da)) - set(os.listdir(do))) == sorted(CLUSTER_FILES)
    for fn in sorted(set(os.listdir(do)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(do / fn):
            assert open(do / fn, "rb").read() == open(da / fn, "rb").read(), fn
    c0, r0 = restate_clusters(t["seqs"], K, t["count"], t["thre"], 13)
    assert 0 < len(r0) < len(t["before"][1])
    len0 = [len(s) for s in t["seqs"]]
    assert open(da / "asm.fa.het_clusters.before.vcf").read() == hetclusters.vcf_text(K, t["thre"], 13, t["names"], len0, t["seqs"], r0)
    mo, ma = messages(po.stdout), messages(pa.stdout)
    extra = [m for m in ma if m.startswith("Het clusters")]
    assert len(extra) == 1 and [m for m in ma if m not in extra] == mo and ma[ma.index(extra[0]) - 1].startswith("Mixed insertions")


def test_kmerqc_with_the_flag(runs, truth, tmp_path):
    from jasper_amd import hetclusters
    d = runs["clusters"][0]
    t = truth
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(t["thre"]), "--indels"]
    p = cli(d, base + ["-o", str(tmp_path / "qc"), "--het-clusters"], module="jasper_amd.kmerqc")
    c0, r0 = t["before"]
    len0 = [len(s) for s in t["seqs"]]
    assert open(tmp_path / "qc.het_clusters.tsv").read() == hetclusters.het_clusters_tsv_text(t["names"], [("asm", len0, c0)])
    assert open(tmp_path / "qc.het_clusters.vcf").read() == open(d / "asm.fa.het_clusters.before.vcf").read()
    assert [m for m in messages(p.stdout) if m.startswith("Het")] == ["Het clusters: %s in %s.het_clusters.vcf" % (hetclusters.stage_log_text(c0), tmp_path / "qc")]
    # without the flag: the same other files, no het-cluster file, no such line
    p0 = cli(d, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    mine = sorted(fn[3:] for fn in os.listdir(tmp_path) if fn.startswith("qc."))
    theirs = sorted(fn[3:] for fn in os.listdir(tmp_path) if fn.startswith("q0."))
    assert sorted(set(mine) - set(theirs)) == ["het_clusters.tsv", "het_clusters.vcf"] and set(theirs) <= set(mine)
    for ext in theirs:
        assert open(str(tmp_path / "q0.") + ext, "rb").read() == open(str(tmp_path / "qc.") + ext, "rb").read(), ext
    m0 = messages(p0.stdout)
    assert not [m for m in m0 if "Het clusters" in m]
    assert [m for m in messages(p.stdout) if not m.startswith("Het clusters")] == [m.replace(str(tmp_path / "q0"), str(tmp_path / "qc")) for m in m0]
