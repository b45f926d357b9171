"""GPU: `python -m jasper_amd.cli ... --compound` and `python -m jasper_amd.kmerqc ... --compound` on the golden cases cluster_k25 and
diploid_k25 (their reads and their contig, written out as the tools' inputs).  The histogram of diploid_k25's small read set has no
local minimum (src/jellyfish.py exits 1 on it, meta.json); the driver, as src/jasper.sh:195-206, then uses the threshold.txt it finds,
so that case gets its own threshold written there, as test_gpu_cli_variants.py does it.

With the flag the three compound files and the new log line equal jasper_amd/compound.py's texts (checked on hand-made records in
test_compound_host.py) of what the restatement of test_compound_host.py lists over a Python dict of the reads' k-mers; with --report as
well the report files are those of --report alone; without the flag the same command writes what it writes today."""
import os

import pytest

from golden_util import Case
from test_compound_host import restate_compound
from test_gpu_cli_spectra import REPORT_FILES, cli, messages, read_fasta
from test_gpu_copies import dict_counter, kmer_dict

pytestmark = pytest.mark.gpu
K = 25
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "2"]
COMPOUND_FILES = ("asm.fa.compound.after.vcf", "asm.fa.compound.before.vcf", "asm.fa.compound.tsv")


def write_inputs(d, case):
    c = Case(case)
    _, seqs = c.batch()
    with open(d / "reads.fq", "wb") as f:
        f.write(c.reads_text())
    with open(d / "asm.fa", "w") as f:
        for i, s in enumerate(seqs):
            f.write(">ctg%d of=%s\n" % (i + 1, case))
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + "\n")
    if case == "diploid_k25":
        with open(d / "threshold.txt", "w") as f:
            f.write("%d\n" % c.thre)


def run_modes(tmp_path_factory, case, modes):
    out = {}
    for mode, flags in modes:
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d, case)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


@pytest.fixture(scope="module", params=["cluster_k25", "diploid_k25"])
def runs(hip, tmp_path_factory, request):
    """the driver on either case: without the flag, with it, with --report, and with both"""
    out = run_modes(tmp_path_factory, request.param, (("plain", []), ("compound", ["--compound"] + (["--compound-max-len", "64"] if request.param == "diploid_k25" else [])),
                                                      ("report", ["--report"]), ("both", ["--compound", "--report"])))
    out["case"] = request.param
    return out


@pytest.fixture(scope="module")
def truth(runs):
    d = runs["compound"][0]
    thre = int(open(d / "threshold.txt").read().split()[0])
    count = dict_counter(kmer_dict(open(d / "reads.fq", "rb").read().split(b"\n")[1::4], K))
    names, seqs = read_fasta(d / "asm.fa")
    pnames, pseqs = read_fasta(d / "asm.fa.polished.fasta")
    assert pnames == names and thre >= 1 and (runs["case"] != "diploid_k25" or thre == Case("diploid_k25").thre)
    return dict(thre=thre, names=names, seqs=seqs, pseqs=pseqs, before=restate_compound(seqs, K, count, thre, 64), after=restate_compound(pseqs, K, count, thre, 64))


def test_compound_files_and_log_line(runs, truth):
    from jasper_amd import compound
    (d0, p0), (d1, p1) = runs["plain"], runs["compound"]
    t = truth
    (c0, r0), (c1, r1) = t["before"], t["after"]
    assert len(r0) >= 1                                       # the input holds what the flag is for
    len0, len1 = [len(s) for s in t["seqs"]], [len(s) for s in t["pseqs"]]
    assert open(d1 / "asm.fa.compound.tsv").read() == compound.compound_tsv_text(t["names"], [("before", len0, c0), ("after", len1, c1)])
    assert open(d1 / "asm.fa.compound.before.vcf").read() == compound.vcf_text(K, t["thre"], 64, t["names"], len0, t["seqs"], r0)
    assert open(d1 / "asm.fa.compound.after.vcf").read() == compound.vcf_text(K, t["thre"], 64, t["names"], len1, t["pseqs"], r1)
    # without the flag: the same files but the three, byte for byte, and the same log lines but one, which comes last of the extensions
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(COMPOUND_FILES) and set(os.listdir(d0)) <= set(os.listdir(d1))
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if m.startswith("Compound scan")]
    assert extra == [compound.log_text(c0, c1)] and [m for m in m1 if m not in extra] == m0
    assert m1.index(extra[0]) == len(m1) - 2 and m1[-1].startswith("Polished sequence is in")


def test_with_report_the_report_files_are_those_of_report_alone(runs):
    (dr, pr), (db, pb), (dc, _) = runs["report"], runs["both"], runs["compound"]
    assert sorted(set(os.listdir(db)) - set(os.listdir(dr))) == sorted(COMPOUND_FILES)
    for fn in REPORT_FILES:
        assert open(db / fn, "rb").read() == open(dr / fn, "rb").read(), fn
    for fn in COMPOUND_FILES:
        assert open(db / fn, "rb").read() == open(dc / fn, "rb").read(), fn
    mr, mb = messages(pr.stdout), messages(pb.stdout)
    assert [m for m in mb if not m.startswith("Compound scan")] == mr and len(mb) == len(mr) + 1


def test_kmerqc_with_the_flag(runs, truth, tmp_path):
    from jasper_amd import compound
    d = runs["compound"][0]
    t = truth
    base = ["-a", "asm.fa", "-j", "mer_counts%d.jf" % K, "--threshold", str(t["thre"])]
    p = cli(d, base + ["-o", str(tmp_path / "qc"), "--compound"], module="jasper_amd.kmerqc")
    c0, r0 = t["before"]
    len0 = [len(s) for s in t["seqs"]]
    assert open(tmp_path / "qc.compound.tsv").read() == compound.compound_tsv_text(t["names"], [("asm", len0, c0)])
    assert open(tmp_path / "qc.compound.vcf").read() == open(d / "asm.fa.compound.before.vcf").read()
    assert [m for m in messages(p.stdout) if m.startswith("Compound")] == ["Compound scan: %s in %s.compound.vcf" % (compound.stage_log_text(c0), tmp_path / "qc")]
    # without the flag: the same report files, no compound file, no such line
    p0 = cli(d, base + ["-o", str(tmp_path / "q0")], module="jasper_amd.kmerqc")
    for ext in (".kmer_qv.tsv", ".unreliable.bed"):
        assert open(str(tmp_path / "q0") + ext, "rb").read() == open(str(tmp_path / "qc") + ext, "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["q0.kmer_qv.tsv", "q0.unreliable.bed", "qc.compound.tsv", "qc.compound.vcf", "qc.kmer_qv.tsv", "qc.unreliable.bed"]
    m0 = messages(p0.stdout)
    assert not [m for m in m0 if "Compound" in m] and [m for m in messages(p.stdout) if not m.startswith("Compound")] == [m.replace(str(tmp_path / "q0"), str(tmp_path / "qc")) for m in m0]


def test_kmerqc_on_diploid_k25(hip, tmp_path):
    """reads counted by kmerqc itself, the case's own threshold; expected from the case's dump as `jellyfish dump -c` printed it"""
    from jasper_amd import compound
    c = Case("diploid_k25")
    write_inputs(tmp_path, "diploid_k25")
    names, seqs = read_fasta(tmp_path / "asm.fa")
    counts, recs = restate_compound(seqs, c.k, dict_counter({key.encode(): v for key, v in c.dump().items()}), c.thre, 7)
    assert len(recs) == 2 and counts == [(2, 2, 2, 1, 0)] and c.k == K      # (at max_len 7 the third cluster of the case is a long run)
    base = ["-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "--threshold", str(c.thre)]
    p = cli(tmp_path, base + ["--compound", "--compound-max-len", "7"], module="jasper_amd.kmerqc")
    lens = [len(s) for s in seqs]
    assert open(tmp_path / "asm.fa.compound.tsv").read() == compound.compound_tsv_text(names, [("asm", lens, counts)])
    assert open(tmp_path / "asm.fa.compound.vcf").read() == compound.vcf_text(K, c.thre, 7, names, lens, seqs, recs)
    assert [m for m in messages(p.stdout) if m.startswith("Compound")] == ["Compound scan: %s in asm.fa.compound.vcf" % compound.stage_log_text(counts)]
    report = {fn: open(tmp_path / fn, "rb").read() for fn in ("asm.fa.kmer_qv.tsv", "asm.fa.unreliable.bed")}
    cli(tmp_path, base + ["-o", "q0"], module="jasper_amd.kmerqc")
    assert [open(tmp_path / fn, "rb").read() for fn in ("q0.kmer_qv.tsv", "q0.unreliable.bed")] == list(report.values())
    assert not [fn for fn in os.listdir(tmp_path) if fn.startswith("q0.compound")]
