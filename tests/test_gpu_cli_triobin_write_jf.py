"""GPU: `python -m jasper_amd.triobin --write-jf` as a child process, on the haplotype fixture (tests/markers_ref.py: make_haps) and on the
trio fixture (test_gpu_cli_triobin.Truth).  Each database is loaded with KmerTable.from_jf and compared, as a dict, with the
restatement: the Counter of canonical k-mer strings over the reads the restatement bins <that bin> or unknown.  Nothing expected here
comes from the code under test.  That the fixture is no vacuous input is asserted on the restatement alone in test_bintables_host.py."""
import collections
import os
import re
import subprocess
import sys

import pytest

import layout_util as lu
import markers_ref as mr
import readbins_ref as ref
from test_gpu_cli_spectra import ROOT, cli, messages
from test_gpu_cli_triobin import PARENTS, THRESHOLDS, Truth
from test_gpu_cli_triobin_haps import HAPS, haps, inputs, made_names      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
K = ref.TRIO_K
CHILD = ["--child-threshold", str(mr.HAPS_THRE)]


def databases(reads, bins, names):
    """the restatement: reads = per input [(name, sequence)], bins = per input the bin names -> {bin: Counter} for the first two bins:
    the k-mers of the reads binned that bin or unknown, = all reads - the other bin"""
    per = {b: collections.Counter() for b in names}
    for fr, fb in zip(reads, bins):
        for (_, s), b in zip(fr, fb):
            per[b].update(lu.kmer_counter(s, K))
    everything = per[names[0]] + per[names[1]] + per[names[2]]
    out = {names[0]: everything - per[names[1]], names[1]: everything - per[names[0]]}
    assert out[names[0]] == per[names[0]] + per[names[2]] and out[names[1]] == per[names[1]] + per[names[2]]
    return {b: dict(c) for b, c in out.items()}


def jf_dict(path):
    from jasper_amd import KmerTable
    t = KmerTable.from_jf(str(path))
    try:
        assert t.k == K
        return lu.table_dict(t)
    finally:
        t.close()


def header_cmdline(path):
    import json
    with open(path, "rb") as f:
        hlen = int(f.read(9))
        return json.loads(f.read(hlen).rstrip(b"\0").decode())["cmdline"]


def check_databases(d, prefix, want, names):
    for b in names[:2]:
        got = jf_dict(d / ("%s.%s.jf" % (prefix, b)))
        assert got == want[b], (b, lu._diff(got, want[b]))
    assert not [fn for fn in os.listdir(os.path.dirname(d / prefix) or d) if fn.endswith(".tmp")]


def check_log_line(p, prefix, want, reads, bins, names):
    log = messages(p.stdout)
    assert len(log) == 3 and log[1].startswith("Read bins:") and log[2].startswith("K-mer databases:"), log
    flat = [(len(s), b) for fr, fb in zip(reads, bins) for (_, s), b in zip(fr, fb)]
    for b in names[:2]:
        mine = [n for n, rb in flat if rb in (b, names[2])]
        assert "%s.%s.jf of the %s and %s reads: %d reads, %d bases, %d distinct k-mers, %d occurrences" % (
            prefix, b, b, names[2], len(mine), sum(mine), len(want[b]), sum(want[b].values())) in log[2], (b, log[2])


# ---- assembly mode --------------------------------------------------------------------------------------------------------------------
def test_solid_markers_keep_the_reads_table(inputs, haps):
    """--markers solid: R is the child's table the markers were selected with.  With --write-reads and --per-read beside it: the other
    files are what they are without the flag"""
    d, (h, truths) = inputs, haps
    t = truths["solid"]
    paths, reads = ["R1.fq", "R2.fq"], [h["r1"], h["r2"]]
    _, _, bins = t.files(paths, ["r1", "r2"])
    want = databases(reads, bins, mr.BINS)
    os.mkdir(d / "jf_solid")
    os.mkdir(d / "jf_solid_without")
    args = ["-r", " ".join(paths), "--per-read", "--write-reads"] + HAPS + CHILD
    p = cli(d, args + ["-o", "jf_solid/p", "--write-jf"], env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    q = cli(d, args + ["-o", "jf_solid_without/p"], module="jasper_amd.triobin")
    assert sorted(os.listdir(d / "jf_solid")) == sorted(made_names("p") + ["p.hap1.jf", "p.hap2.jf"])
    assert sorted(os.listdir(d / "jf_solid_without")) == made_names("p")                  # without the flag: the files that were
    for fn in made_names("p"):
        assert open(d / "jf_solid" / fn, "rb").read() == open(d / "jf_solid_without" / fn, "rb").read(), fn
    assert [m.replace("jf_solid/p", "jf_solid_without/p") for m in messages(p.stdout)[:2]] == messages(q.stdout)
    check_databases(d / "jf_solid", "p", want, mr.BINS)
    check_log_line(p, "jf_solid/p", want, reads, bins, mr.BINS)
    assert header_cmdline(d / "jf_solid" / "p.hap1.jf") == ["count", "-C", "-m", str(K), "-o", "jf_solid/p.hap1.jf", "R1.fq", "R2.fq"]
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("[triobin] write-jf:")]
    assert len(line) == 1 and "[triobin] write-jf" not in q.stderr
    # two sinks: the reads of hap1 and of hap2 were gathered, each with a separator byte, and nothing else
    flat = [(len(s), b) for fr, fb in zip(reads, bins) for (_, s), b in zip(fr, fb)]
    gathered = sum(n + 1 for n, b in flat if b != "unknown")
    assert "for %d bytes;" % gathered in line[0], line[0]
    everything = len(databases(reads, [["unknown"] * len(fb) for fb in bins], mr.BINS)["hap1"])
    m = re.search(r"hap1 [\d.]+ \(swept (\d+), matched (\d+), dropped (\d+), underflow (\d+), kept (\d+)\)", line[0])
    assert m and int(m.group(1)) == everything and int(m.group(4)) == 0 and int(m.group(5)) == len(want["hap1"]), line[0]


def test_all_markers_count_the_reads_as_a_third_sink(inputs, haps):
    """--markers all counts no child table: R is a sink of the pass.  Without --write-reads"""
    d, (h, truths) = inputs, haps
    t = truths["all"]
    paths, reads = ["R1.fq", "R2.fq"], [h["r1"], h["r2"]]
    _, _, bins = t.files(paths, ["r1", "r2"])
    want = databases(reads, bins, mr.BINS)
    os.mkdir(d / "jf_all")
    p = cli(d, ["-r", " ".join(paths), "-o", "jf_all/p", "--markers", "all", "--write-jf"] + HAPS, env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    assert sorted(os.listdir(d / "jf_all")) == ["p.hap1.jf", "p.hap2.jf", "p.readbins.tsv"]
    check_databases(d / "jf_all", "p", want, mr.BINS)
    check_log_line(p, "jf_all/p", want, reads, bins, mr.BINS)
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("[triobin] write-jf:")]
    flat = [(len(s), b) for fr, fb in zip(reads, bins) for (_, s), b in zip(fr, fb)]
    assert len(line) == 1 and "for %d bytes;" % (sum(n + 1 for n, _ in flat) + sum(n + 1 for n, b in flat if b != "unknown")) in line[0], line[0]


def test_paired(inputs, haps):
    d, (h, truths) = inputs, haps
    t = truths["solid"]
    paths, reads = ["R1.fq", "R2.fq"], [h["r1"], h["r2"]]
    _, _, bins = t.files(paths, ["r1", "r2"], paired=True)
    assert bins != t.files(paths, ["r1", "r2"])[2]
    want = databases(reads, bins, mr.BINS)
    os.mkdir(d / "jf_paired")
    p = cli(d, ["-r", " ".join(paths), "-o", "jf_paired/p", "--paired", "--write-jf"] + HAPS + CHILD, module="jasper_amd.triobin")
    check_databases(d / "jf_paired", "p", want, mr.BINS)
    check_log_line(p, "jf_paired/p", want, reads, bins, mr.BINS)


def test_every_device_path_on_gz_input(inputs, haps):
    """--reader device --gz device (and --route device --write-gz --deflate device for the bin files beside them): the sequences are
    parsed, packed, gathered and counted without visiting the host; once with R kept, once with R as a sink"""
    d, (h, truths) = inputs, haps
    paths, reads = ["R1.fq.gz", "R2.fq.gz"], [h["r1"], h["r2"]]
    device = ["--reader", "device", "--gz", "device"]
    for sub, markers, more in (("jf_dev_solid", "solid", CHILD + ["--write-reads", "--route", "device", "--write-gz", "--deflate", "device"]), ("jf_dev_all", "all", [])):
        _, _, bins = truths[markers].files(paths, ["r1", "r2"])
        want = databases(reads, bins, mr.BINS)
        os.mkdir(d / sub)
        p = cli(d, ["-r", " ".join(paths), "-o", sub + "/p", "--markers", markers, "--write-jf"] + device + more + HAPS, env={"JASPER_TRIOBIN_CHUNK": "100000"},
                module="jasper_amd.triobin")
        check_databases(d / sub, "p", want, mr.BINS)
        check_log_line(p, sub + "/p", want, reads, bins, mr.BINS)
    # a plain file through the device reader, without a gz session
    _, _, bins = truths["all"].files(["R1.fq", "R2.fq"], ["r1", "r2"])
    os.mkdir(d / "jf_dev_plain")
    cli(d, ["-r", "R1.fq R2.fq", "-o", "jf_dev_plain/p", "--markers", "all", "--write-jf", "--reader", "device"] + HAPS, module="jasper_amd.triobin")
    check_databases(d / "jf_dev_plain", "p", databases(reads, bins, mr.BINS), mr.BINS)


def test_child_database_and_one_of_other_reads(inputs, haps):
    """--child-jf made from these reads gives the same databases; one made from R1 alone lacks what R2's reads hold: exit status 1, the
    message, and no file at all"""
    from jasper_amd import KmerTable
    d, (h, truths) = inputs, haps
    t = truths["solid"]
    paths, reads = ["R1.fq", "R2.fq"], [h["r1"], h["r2"]]
    _, _, bins = t.files(paths, ["r1", "r2"])
    want = databases(reads, bins, mr.BINS)
    for name, files in (("child_all.jf", paths), ("child_r1.jf", paths[:1])):
        table = KmerTable(K, min_slots=1 << 18)
        table.count_files([str(d / f) for f in files])
        table.write_jf(str(d / name))
        table.close()
    os.mkdir(d / "jf_child")
    p = cli(d, ["-r", " ".join(paths), "-o", "jf_child/p", "--child-jf", "child_all.jf", "--write-jf", "--hap1", "hap1.fa", "--hap2", "hap2.fa"] + CHILD,
            module="jasper_amd.triobin")
    check_databases(d / "jf_child", "p", want, mr.BINS)
    check_log_line(p, "jf_child/p", want, reads, bins, mr.BINS)
    os.mkdir(d / "jf_wrong")
    q = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", " ".join(paths), "-o", "jf_wrong/p", "--child-jf", "child_r1.jf", "--write-jf", "--write-reads",
                        "--hap1", "hap1.fa", "--hap2", "hap2.fa"] + CHILD, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert q.returncode == 1 and "--child-jf is not the database of these reads" in q.stderr, q.stdout + q.stderr
    assert os.listdir(d / "jf_wrong") == []
    # a database --write-jf would write over is refused before anything is opened
    q = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", " ".join(paths), "-o", "child_all", "--child-jf", "child_all.hap1.jf", "--write-jf",
                        "--hap1", "hap1.fa", "--hap2", "hap2.fa"] + CHILD, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert q.returncode == 1 and "child_all.hap1.jf" in q.stderr and not os.path.exists(d / "child_all.hap1.jf")


# ---- trio mode ------------------------------------------------------------------------------------------------------------------------
def test_trio_mode(hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin_write_jf_trio")
    t = Truth()
    t.write(d)
    paths, reads = ["z/R1.fastq.gz", "z/R2_crlf.fastq"], [t.trio["r1"], t.trio["r2"]]
    _, _, bins = t.files(paths, ["r1", "r2"])
    want = databases(reads, bins, ref.BINS)
    for sub, more in (("host", []), ("tables", ["--marker-tables", "--reader", "device", "--gz", "device"])):
        os.mkdir(d / sub)
        p = cli(d, ["-r", " ".join(paths), "-o", sub + "/p", "--write-jf"] + more + PARENTS + THRESHOLDS, module="jasper_amd.triobin")
        assert sorted(os.listdir(d / sub)) == ["p.mat.jf", "p.pat.jf", "p.readbins.tsv"]
        check_databases(d / sub, "p", want, ref.BINS)
        check_log_line(p, sub + "/p", want, reads, bins, ref.BINS)
    # a file that has changed between the passes cannot be provoked from outside a run; the record count's check is the host test's


# ---- end to end: the driver polishes the same from the database as from the bin files ---------------------------------------------------
def test_the_driver_polishes_the_same_from_the_database(inputs, haps):
    """two fresh directories; the fixture's reads cover every k-mer 10 or 20 times, so their histogram has no error peak for the
    solid-k-mer rule to descend from: both runs are given the threshold in threshold.txt, which the driver keeps when the rule
    derives none"""
    d, _ = inputs, haps
    os.mkdir(d / "e2e")
    cli(d, ["-r", "R1.fq R2.fq", "-o", "e2e/p", "--write-jf", "--write-reads"] + HAPS + CHILD, module="jasper_amd.triobin")
    out = {}
    for sub, source in (("from_jf", ["-j", "../e2e/p.hap1.jf"]),
                        ("from_reads", ["-r", " ".join("../e2e/p.%s.%s" % (b, f) for f in ("R1.fq", "R2.fq") for b in ("hap1", "unknown"))])):
        os.mkdir(d / sub)
        (d / sub / "hap1.fa").write_bytes(open(d / "hap1.fa", "rb").read())
        (d / sub / "threshold.txt").write_text("%d\n" % mr.HAPS_THRE)
        cli(d / sub, ["-a", "hap1.fa", "-k", str(K), "-p", "2"] + source)
        out[sub] = {fn: open(d / sub / fn, "rb").read() for fn in os.listdir(d / sub) if fn.endswith(".polished.fasta") or fn.endswith(".fixes.csv")}
    assert sorted(out["from_jf"]) == ["hap1.fa.fixes.csv", "hap1.fa.polished.fasta"], sorted(os.listdir(d / "from_jf"))
    assert out["from_jf"] == out["from_reads"]
    assert out["from_jf"]["hap1.fa.fixes.csv"].count(b"\n") > 3, "the haplotype's planted errors are repaired: no vacuous comparison"
