"""GPU: `python -m jasper_amd.triobin --hap1 .. --hap2 ..` as a child process on the synthetic trio's two haplotypes as the assemblies
(tests/markers_ref.py: make_haps -- hap1 carries assembly errors), and trio mode with --marker-tables.  Every file equals, byte for byte,
what the restatement gives from Python dicts; nothing expected here comes from the code under test.  That the fixture is no vacuous
input is asserted on the restatement alone in test_markers_host.py."""
import gzip
import os
import subprocess
import sys

import pytest

import markers_ref as mr
import readbins_ref as ref
from test_gpu_cli_spectra import ROOT, cli, messages
from test_gpu_cli_triobin import PARENTS, THRESHOLDS, Truth

pytestmark = pytest.mark.gpu
K = ref.TRIO_K
THRE = mr.HAPS_THRE
HAPS = ["--hap1", "hap1.fa", "--hap2", "hap2.fa", "-k", str(K)]
PER_READ = ["--per-read", "--write-reads"]
DEVICE = ["--reader", "device", "--gz", "device", "--route", "device", "--write-gz", "--deflate", "device"]


@pytest.fixture(scope="module")
def haps():
    h = mr.make_haps()
    reads = {"r1": h["r1"], "r2": h["r2"]}
    return h, {m: mr.Haps(K, [h["hap1"]], [h["hap2"]], reads, m, THRE) for m in ("solid", "all")}


@pytest.fixture(scope="module")
def inputs(hip, haps, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin_haps")
    h = haps[0]
    (d / "hap1.fa").write_bytes(mr.fasta(b"h1 first haplotype", h["hap1"]))
    (d / "hap2.fa").write_bytes(mr.fasta(b"h2", h["hap2"], 61))
    for f, w in (("R1.fq", "r1"), ("R2.fq", "r2")):
        (d / f).write_bytes(ref.fastq_text(h[w]))
        with gzip.open(d / (f + ".gz"), "wb") as z:
            z.write(ref.fastq_text(h[w]))
    return d


def records(reads):
    return [ref.fastq_text([r]) for r in reads]


def check_outputs(d, prefix, truth, paths, reads, gz=False):
    """both tables and the six bin files of a run on `paths` (the r1 and the r2 file) under `prefix`"""
    want_tsv, want_reads, bins = truth.files(paths, ["r1", "r2"])
    assert open(d / (prefix + ".readbins.tsv")).read() == want_tsv
    assert open(d / (prefix + ".readbins.reads.tsv")).read() == want_reads
    for base, w, fb in (("R1.fq", "r1", bins[0]), ("R2.fq", "r2", bins[1])):
        for b in mr.BINS:
            fn = d / ("%s.%s.%s%s" % (prefix, b, base, ".gz" if gz else ""))
            data = gzip.open(fn, "rb").read() if gz else open(fn, "rb").read()
            assert data == b"".join(r for r, rb in zip(records(reads[w]), fb) if rb == b), (base, b)
    return bins


def made_names(prefix, gz=False):
    return sorted(["%s.readbins.tsv" % prefix, "%s.readbins.reads.tsv" % prefix] +
                  ["%s.%s.%s%s" % (prefix, b, f, ".gz" if gz else "") for b in mr.BINS for f in ("R1.fq", "R2.fq")])


def check_log(p, truth, markers, origin):
    log = messages(p.stdout)
    assert len(log) == 2, log
    assert "Haplotype read binning with k = %d: markers %s, %s;" % (K, markers, origin) in log[0]
    assert "%d hap1 and %d hap2 markers, of %d and %d k-mers private" % ((truth.m_total, truth.p_total) + truth.private) in log[0]
    return log


# ---- assembly mode ------------------------------------------------------------------------------------------------------------------
def test_all_markers_on_plain_files(inputs, haps):
    d, (h, truths) = inputs, haps
    t = truths["all"]
    before = set(os.listdir(d))
    p = cli(d, ["-r", "R1.fq R2.fq", "--markers", "all"] + PER_READ + HAPS, env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    assert sorted(set(os.listdir(d)) - before) == made_names("R1.fq")
    bins = check_outputs(d, "R1.fq", t, ["R1.fq", "R2.fq"], h)
    flat = bins[0] + bins[1]
    log = check_log(p, t, "all", "no child threshold")
    assert "hap1 %d reads" % flat.count("hap1") in log[1] and "hap2 %d reads" % flat.count("hap2") in log[1] and "unknown %d reads" % flat.count("unknown") in log[1]
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("[triobin] select device seconds")]
    assert len(line) == 1 and "hap1 " in line[0] and "hap2 " in line[0]
    assert "(candidates %d, in_absent %d, not_solid %d, selected %d)" % t.m_stats in line[0] and "(candidates %d, in_absent %d, not_solid %d, selected %d)" % t.p_stats in line[0]
    for fn in set(os.listdir(d)) - before:
        os.remove(d / fn)


def test_solid_markers_host_and_device_paths_and_a_database(inputs, haps):
    """--markers solid (the default) on the .gz inputs: the plain run equals the restatement; the run with every device path equals the
    plain run -- the tables as they stand, the bin files after gzip decompression; and a run whose child table comes from a database
    written by the project's own .jf writer equals the counted run"""
    from jasper_amd import KmerTable
    d, (h, truths) = inputs, haps
    t = truths["solid"]
    assert (t.m_total, t.p_total) != (truths["all"].m_total, truths["all"].p_total)
    paths = ["R1.fq.gz", "R2.fq.gz"]
    child = ["--child-threshold", str(THRE)]
    for sub in ("plain", "dev", "jf"):
        os.mkdir(d / sub)
    p = cli(d, ["-r", " ".join(paths), "-o", "plain/p"] + PER_READ + HAPS + child, env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    assert sorted(os.listdir(d / "plain")) == made_names("p")
    check_outputs(d / "plain", "p", t, paths, h)
    log = check_log(p, t, "solid", "child threshold %d (given)" % THRE)
    assert "(candidates %d, in_absent %d, not_solid %d, selected %d)" % t.m_stats in p.stderr
    # every device path, and --marker-tables, which changes nothing here
    q = cli(d, ["-r", " ".join(paths), "-o", "dev/p", "--marker-tables"] + PER_READ + DEVICE + HAPS + child, module="jasper_amd.triobin")
    assert sorted(os.listdir(d / "dev")) == made_names("p", gz=True)
    check_outputs(d / "dev", "p", t, paths, h, gz=True)
    for fn in ("p.readbins.tsv", "p.readbins.reads.tsv"):
        assert open(d / "dev" / fn, "rb").read() == open(d / "plain" / fn, "rb").read()
    assert [m.replace("dev/p", "plain/p") for m in messages(q.stdout)] == log
    # the child's table from a database
    table = KmerTable(K, min_slots=1 << 18)
    table.count_files([str(d / "R1.fq"), str(d / "R2.fq")])
    table.write_jf(str(d / "child.jf"))
    table.close()
    r = cli(d, ["-r", " ".join(paths), "-o", "jf/p", "--child-jf", "child.jf", "-k", "31"] + PER_READ + ["--hap1", "hap1.fa", "--hap2", "hap2.fa"] + child,
            module="jasper_amd.triobin")                                                  # (the database's header decides k, not -k)
    assert sorted(os.listdir(d / "jf")) == made_names("p")
    for fn in os.listdir(d / "jf"):
        assert open(d / "jf" / fn, "rb").read() == open(d / "plain" / fn, "rb").read(), fn
    assert [m.replace("jf/p", "plain/p") for m in messages(r.stdout)] == log


def test_threshold_from_the_histogram(inputs, haps):
    """no --child-threshold: with the noise reads (markers_ref.noise_reads) the reads' histogram has an error peak to descend from, and
    the solid-k-mer rule, restated in markers_ref, derives 2"""
    d, (h, _) = inputs, haps
    reads = {"r1": h["r1"], "r2": h["r2"], "noise": mr.noise_reads()}
    (d / "noise.fq").write_bytes(ref.fastq_text(reads["noise"]))
    child = ref.kmer_dict([s for r in reads.values() for _, s in r], K)
    thre = mr.histo_threshold(child)
    assert thre == 2
    t = mr.Haps(K, [h["hap1"]], [h["hap2"]], reads, "solid", thre)
    os.mkdir(d / "histo")
    p = cli(d, ["-r", "R1.fq R2.fq noise.fq", "-o", "histo/p", "--per-read"] + HAPS, module="jasper_amd.triobin")
    want_tsv, want_reads, _ = t.files(["R1.fq", "R2.fq", "noise.fq"], ["r1", "r2", "noise"])
    assert sorted(os.listdir(d / "histo")) == ["p.readbins.reads.tsv", "p.readbins.tsv"]
    assert open(d / "histo" / "p.readbins.tsv").read() == want_tsv and open(d / "histo" / "p.readbins.reads.tsv").read() == want_reads
    check_log(p, t, "solid", "child threshold %d (from the histogram)" % thre)
    os.remove(d / "noise.fq")


def test_no_threshold_from_the_histogram_and_a_side_without_markers_end_the_run(inputs, haps):
    """the fixture's reads cover every k-mer 10 or 20 times: the solid-k-mer rule finds no descent to follow and derives no threshold"""
    d = inputs
    (d / "hap1_copy.fa").write_bytes(mr.fasta(b"again", haps[0]["hap1"], 70))
    before = set(os.listdir(d))
    for args, message in ((["-r", "R1.fq R2.fq"] + PER_READ + HAPS, "gives no threshold. Please give one with --child-threshold"),
                          (["-r", "R1.fq", "--markers", "all", "--hap1", "hap1.fa", "--hap2", "hap1_copy.fa", "-k", str(K)] + PER_READ, "The haplotypes have no marker k-mers")):
        p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin"] + args, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1 and message in p.stderr, p.stdout + p.stderr
        assert set(os.listdir(d)) == before


# ---- trio mode: --marker-tables ------------------------------------------------------------------------------------------------------
def test_trio_mode_on_marker_tables_writes_the_same_bytes(hip, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin_marker_tables")
    t = Truth()
    t.write(d)
    want_tsv, want_reads, bins = t.files(["R1.fq", "R2.fq"], ["r1", "r2"])
    os.mkdir(d / "with")
    os.mkdir(d / "without")
    args = ["-r", "R1.fq R2.fq"] + PER_READ + PARENTS + THRESHOLDS
    p = cli(d, args + ["-o", "with/p", "--marker-tables"], env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    q = cli(d, args + ["-o", "without/p"], env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    assert open(d / "with" / "p.readbins.tsv").read() == want_tsv and open(d / "with" / "p.readbins.reads.tsv").read() == want_reads
    for w, f, fb in (("r1", "R1.fq", bins[0]), ("r2", "R2.fq", bins[1])):
        for b in ref.BINS:
            assert open(d / "with" / ("p.%s.%s" % (b, f)), "rb").read() == b"".join(r for r, rb in zip(records(t.trio[w]), fb) if rb == b), (f, b)
    assert sorted(os.listdir(d / "with")) == sorted(os.listdir(d / "without")) and len(os.listdir(d / "with")) == 8
    for fn in os.listdir(d / "with"):
        assert open(d / "with" / fn, "rb").read() == open(d / "without" / fn, "rb").read(), fn
    log = messages(p.stdout)
    assert len(log) == 2 and [m.replace("with/p", "without/p") for m in log] == messages(q.stdout)
    assert "%d maternal and %d paternal hap-mers" % (t.m_total, t.p_total) in log[0]
    select = [ln for ln in p.stderr.splitlines() if ln.startswith("[triobin] select device seconds")]
    assert len(select) == 1 and "selected %d)" % t.m_total in select[0] and "selected %d)" % t.p_total in select[0]
    assert "select device seconds" not in q.stderr
    strip = lambda err: [ln.split(":")[0] for ln in err.splitlines() if ln.startswith("[triobin]") and "select device" not in ln]      # noqa: E731
    assert strip(p.stderr) == strip(q.stderr)
    # the device paths run on the marker tables as they run on the parents'
    os.mkdir(d / "dev")
    cli(d, ["-r", "z/R1.fastq.gz R2.fq", "-o", "dev/p", "--marker-tables"] + PER_READ + DEVICE + PARENTS + THRESHOLDS, module="jasper_amd.triobin")
    want_tsv, want_reads, _ = t.files(["z/R1.fastq.gz", "R2.fq"], ["r1", "r2"])
    assert open(d / "dev" / "p.readbins.tsv").read() == want_tsv and open(d / "dev" / "p.readbins.reads.tsv").read() == want_reads
    for w, f, fb in (("r1", "R1.fastq", bins[0]), ("r2", "R2.fq", bins[1])):
        for b in ref.BINS:
            assert gzip.open(d / "dev" / ("p.%s.%s.gz" % (b, f)), "rb").read() == b"".join(r for r, rb in zip(records(t.trio[w]), fb) if rb == b), (f, b)
