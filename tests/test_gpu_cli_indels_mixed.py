"""GPU: `python -m jasper_amd.cli ... --indels --indel-mixed` and `python -m jasper_amd.kmerqc ... --indels --indel-mixed` on a small planted
diploid input: two haplotypes that differ by insertions of mixed strings and by deletions, reads of both, and the first haplotype as the
assembly.

With the flag the three indel files and the new log line equal what this file computes with the restatements of test_indels_host.py and
test_indels_mixed_host.py over a Python dict of the reads' k-mers, with its own left alignment; without it the same command writes what
--indels writes today; with --variants as well the variant files are those of --variants alone."""
import os

import numpy as np
import pytest

from test_gpu_cli_indels import vcf_line
from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_cli_variants import VARIANT_FILES
from test_gpu_copies import dict_counter, kmer_dict
from test_indels_host import restate
from test_indels_mixed_host import plant_strings, random_string, restate_mixed

pytestmark = pytest.mark.gpu
K = 25
MAX_LEN = 8
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2", "--indels", "--indel-max-len", str(MAX_LEN)]
INDEL_FILES = ("asm.fa.indels.after.vcf", "asm.fa.indels.before.vcf", "asm.fa.indels.tsv")
TSV_HEADER = "#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error\tmixed_het\tmixed_error\tcomplex"


def write_inputs(d):
    """two contigs of one haplotype as the assembly (a stretch of the second in lower case); the other haplotype has an insertion of a
    random string or a deletion every 500 bases; 150-base reads of both at 25x each"""
    from jasper_amd import synth
    rng = np.random.default_rng(77)
    h1 = synth.make_genome(rng, 16_000).tobytes()
    events = []
    for i, q in enumerate(range(400, 15_600, 500)):
        L = (2, 3, 1, 8, 5, 4, 7, 6)[i % 8]
        events.append((q, "ins", random_string(rng, L)) if i % 2 == 0 else (q, "del", L))
    h2 = plant_strings(h1, events)
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
    for mode, flags in (("indels", []), ("mixed", ["--indel-mixed"]), ("variants", ["--variants"]), ("all", ["--variants", "--indel-mixed"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d)
        args = [a for a in ARGS if mode != "variants" or a not in ("--indels", "--indel-max-len", str(MAX_LEN))]
        out[mode] = (d, cli(d, args + flags))
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d = runs["mixed"][0]
    thre = int(open(d / "threshold.txt").read().split()[0])
    count = dict_counter(kmer_dict(open(d / "reads.fq", "rb").read().split(b"\n")[1::4], K))
    names, seqs = read_fasta(d / "asm.fa")
    pnames, pseqs = read_fasta(d / "asm.fa.polished.fasta")
    assert pnames == names and thre >= 1
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, before=restate(seqs, K, count, thre, MAX_LEN), after=restate(pseqs, K, count, thre, MAX_LEN),
                mixed_before=restate_mixed(seqs, K, count, thre, MAX_LEN), mixed_after=restate_mixed(pseqs, K, count, thre, MAX_LEN))


def mixed_vcf_line(names, seqs, rec):
    """(sort key, line) of one mixed record: rotated to the left while q > 1 and s[q-1] is a base that folds to y's last base"""
    seq, q, L, y, rmin, amin, kind = rec
    s = seqs[seq]
    while q > 1 and s[q - 1].upper() == y[-1]:
        y, q = y[-1] + y[:-1], q - 1
    ref = s[q - 1].upper()
    line = "%s\t%d\t.\t%s\t%s\t.\t.\tKIND=%s;TYPE=ins;LEN=%d;RC=%d;AC=%d" % (names[seq], q, ref, ref + y, {1: "het", 2: "error"}[kind], L, rmin, amin)
    return (seq, q, 1, L, ref + y), line


def check_tsv(text, names, stages):
    want = []
    for i, n in enumerate(names):
        for stage, seqs, counts, mc in stages:
            want.append((n, stage, len(seqs[i])) + tuple(counts[i]) + tuple(mc[i]))
    for stage, seqs, counts, mc in stages:
        want.append(("*", stage, sum(len(s) for s in seqs)) + tuple(sum(c[j] for c in counts) for j in range(4)) + tuple(sum(c[j] for c in mc) for j in range(3)))
    lines = text.splitlines()
    assert lines[0] == TSV_HEADER and text.endswith("\n")
    assert lines[1:] == ["\t".join(str(v) for v in w) for w in want]


def check_vcf(text, names, seqs, recs, mixed):
    lines = text.splitlines()
    assert lines[1].endswith("max_len=%d, mixed" % MAX_LEN) and any("ins: the reads hold LEN more bases" in ln for ln in lines if ln.startswith("##INFO=<ID=TYPE"))
    head = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    assert lines[head + 1:] == [ln for _, ln in sorted([vcf_line(names, seqs, r) for r in recs] + [mixed_vcf_line(names, seqs, r) for r in mixed])]


def test_mixed_files_and_log_line(runs, truth):
    (d0, p0), (d1, p1) = runs["indels"], runs["mixed"]
    t = truth
    (c0, r0), (c1, r1), (mc0, mr0), (mc1, mr1) = t["before"], t["after"], t["mixed_before"], t["mixed_after"]
    # the input holds what the flag is for, on both contigs and under lower case
    assert len(mr0) >= 10 and {r[0] for r in mr0} == {0, 1} and {r[6] for r in mr0} == {1}
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))
    for fn in sorted(os.listdir(d0)):
        if os.path.isfile(d0 / fn) and fn not in INDEL_FILES and not fn.endswith(".jf"):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    check_tsv(open(d1 / "asm.fa.indels.tsv").read(), t["names"], [("before", t["seqs"], c0, mc0), ("after", t["pseqs"], c1, mc1)])
    check_vcf(open(d1 / "asm.fa.indels.before.vcf").read(), t["names"], t["seqs"], r0, mr0)
    check_vcf(open(d1 / "asm.fa.indels.after.vcf").read(), t["names"], t["pseqs"], r1, mr1)
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if m.startswith("Mixed insertions")]
    assert len(extra) == 1 and [m for m in m1 if m not in extra] == m0
    assert m1[m1.index(extra[0]) - 1].startswith("Indel scan:")
    assert extra[0] == "Mixed insertions: before polishing %d het and %d error mixed insertions, %d complex sites; after polishing %d het and %d error " \
                       "mixed insertions, %d complex sites" % tuple(sum(c[j] for c in cs) for cs in (mc0, mc1) for j in range(3))


def test_without_the_flag_the_files_are_those_of_indels(runs, truth):
    """the run without --indel-mixed against the same-base restatement: the header, the source line and every row are today's"""
    from test_gpu_cli_indels import TSV_HEADER as OLD_HEADER
    d0 = runs["indels"][0]
    t = truth
    tsv = open(d0 / "asm.fa.indels.tsv").read().splitlines()
    assert tsv[0] == OLD_HEADER and all(len(ln.split("\t")) == 7 for ln in tsv)
    for fn, seqs, recs in (("asm.fa.indels.before.vcf", t["seqs"], t["before"][1]), ("asm.fa.indels.after.vcf", t["pseqs"], t["after"][1])):
        lines = open(d0 / fn).read().splitlines()
        assert lines[1] == "##source=jasper_amd indel scan, k=%d, threshold=%d, max_len=%d" % (K, t["thre"], MAX_LEN)
        assert any("ins: the reads hold LEN more copies of one base" in ln for ln in lines)
        head = lines.index("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
        assert lines[head + 1:] == [ln for _, ln in sorted(vcf_line(t["names"], seqs, r) for r in recs)]
    assert not [m for m in messages(runs["indels"][1].stdout) if "Mixed" in m]


def test_variants_with_both_flags_writes_the_variant_files_of_variants_alone(runs):
    (dv, _), (da, pa), (dm, _) = runs["variants"], runs["all"], runs["mixed"]
    assert sorted(set(os.listdir(da)) - set(os.listdir(dv))) == sorted(INDEL_FILES)
    for fn in VARIANT_FILES:
        assert open(da / fn, "rb").read() == open(dv / fn, "rb").read(), fn
    for fn in INDEL_FILES:
        assert open(da / fn, "rb").read() == open(dm / fn, "rb").read(), fn
    assert len([m for m in messages(pa.stdout) if m.startswith("Mixed insertions")]) == 1


def test_kmerqc_with_the_flag(runs, truth, tmp_path):
    d = runs["mixed"][0]
    t = truth
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(t["thre"]), "--indels", "--indel-max-len", str(MAX_LEN)]
    p = cli(d, base + ["-o", str(tmp_path / "qc"), "--indel-mixed"], module="jasper_amd.kmerqc")
    driver = open(d / "asm.fa.indels.tsv").read().splitlines()
    want = [driver[0]] + [ln.replace("\tbefore\t", "\tasm\t", 1) for ln in driver[1:] if "\tbefore\t" in ln]
    assert open(tmp_path / "qc.indels.tsv").read().splitlines() == want
    assert open(tmp_path / "qc.indels.vcf").read() == open(d / "asm.fa.indels.before.vcf").read()
    mc0 = t["mixed_before"][0]
    assert [m for m in messages(p.stdout) if m.startswith("Mixed")] == ["Mixed insertions: %d het and %d error mixed insertions, %d complex sites in %s.indels.vcf" % (
        tuple(sum(c[j] for c in mc0) for j in range(3)) + (tmp_path / "qc",))]
    # without the flag: the files of the driver's run without it
    p = cli(d, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    d0 = runs["indels"][0]
    assert open(tmp_path / "q0.indels.vcf").read() == open(d0 / "asm.fa.indels.before.vcf").read()
    assert not [m for m in messages(p.stdout) if "Mixed" in m]
