"""GPU: `python -m jasper_amd.triobin --reader device` as a child process on the synthetic trio of test_gpu_cli_triobin.py, with
JASPER_TRIOBIN_CHUNK small enough that every file is several blocks and a block's end falls inside records.  Every file equals, byte for
byte, what that module's Truth builds from the restatement and the rule -- nothing expected here comes from the code under test -- and
what the same command writes with --reader host."""
import os
import subprocess
import sys

import pytest

import readbins_ref as ref
from test_gpu_cli_spectra import ROOT, cli
from test_gpu_cli_triobin import PARENTS, THRESHOLDS, Truth, check_read_files

pytestmark = pytest.mark.gpu
CHUNK = 150000                  # the FASTQ files hold about 490 kB, the FASTA file about 240 kB
ENV = {"JASPER_TRIOBIN_CHUNK": str(CHUNK), "JASPER_AMD_TIMING": "1"}
WIDTH = 60


@pytest.fixture(scope="module")
def truth():
    return Truth()


def fasta_records(reads):
    """multi-line FASTA: lines of WIDTH bases, the last one shorter; an empty read is a header alone"""
    return [b">" + name.encode() + b" len=%d\n" % len(s) + b"".join(s[i:i + WIDTH] + b"\n" for i in range(0, len(s), WIDTH)) for name, s in reads]


@pytest.fixture(scope="module")
def inputs(hip, truth, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin_reader")
    truth.write(d)
    (d / "child.fa").write_bytes(b"".join(fasta_records(truth.trio["r2"])))
    for fn in ("R1.fq", "R2.fq", "z/R2_crlf.fastq", "child.fa"):
        assert os.path.getsize(d / fn) > 1.5 * CHUNK, fn       # several blocks each
    return d


def run_both(d, args, out_dir):
    """the command with --reader device and with --reader host, each into its own directory -> {reader: {file: bytes}}"""
    got = {}
    for reader in ("device", "host"):
        os.mkdir(d / (out_dir + reader))
        p = cli(d, args + ["--reader", reader, "-o", "%s%s/pfx" % (out_dir, reader)] + PARENTS + THRESHOLDS, env=ENV, module="jasper_amd.triobin")
        assert "[triobin] read_bins device seconds" in p.stderr
        assert ("[triobin] read_text index + pack device seconds" in p.stderr) == (reader == "device")
        got[reader] = {fn: open(d / (out_dir + reader) / fn, "rb").read() for fn in os.listdir(d / (out_dir + reader))}
    assert got["device"] == got["host"]
    return got["device"]


def test_per_read_and_write_reads(inputs, truth):
    d, t = inputs, truth
    want_tsv, want_reads, bins = t.files(["R1.fq", "R2.fq"], ["r1", "r2"])
    got = run_both(d, ["-r", "R1.fq R2.fq", "--per-read", "--write-reads"], "a_")
    assert sorted(got) == sorted(["pfx.readbins.tsv", "pfx.readbins.reads.tsv"] + ["pfx.%s.%s" % (b, f) for b in ref.BINS for f in ("R1.fq", "R2.fq")])
    assert got["pfx.readbins.tsv"].decode() == want_tsv and got["pfx.readbins.reads.tsv"].decode() == want_reads
    for f, w, fb in (("R1.fq", "r1", bins[0]), ("R2.fq", "r2", bins[1])):
        check_read_files(d / "a_device", "pfx", f, ref.fastq_text(t.trio[w]), b"\n", fb)


def test_pairs_gz_and_crlf(inputs, truth):
    d, t = inputs, truth
    paths = ["z/R1.fastq.gz", "z/R2_crlf.fastq"]
    want_tsv, want_reads, bins = t.files(paths, ["r1", "r2"], paired=True, min_markers=2)
    got = run_both(d, ["-r", " ".join(paths), "--paired", "--per-read", "--write-reads", "--min-markers", "2", "--batch-bases", "300"], "b_")
    assert got["pfx.readbins.tsv"].decode() == want_tsv and got["pfx.readbins.reads.tsv"].decode() == want_reads
    check_read_files(d / "b_device", "pfx", "R1.fastq", ref.fastq_text(t.trio["r1"]), b"\n", bins[0])
    check_read_files(d / "b_device", "pfx", "R2_crlf.fastq", ref.fastq_text(t.trio["r2"], b"\r\n"), b"\r\n", bins[1])


def test_multi_line_fasta(inputs, truth):
    d, t = inputs, truth
    want_tsv, want_reads, bins = t.files(["child.fa"], ["r2"])
    got = run_both(d, ["-r", "child.fa", "--per-read", "--write-reads"], "c_")
    assert got["pfx.readbins.tsv"].decode() == want_tsv and got["pfx.readbins.reads.tsv"].decode() == want_reads
    recs = fasta_records(t.trio["r2"])
    assert any(r.count(b"\n") == 1 for r in recs) and any(r.count(b"\n") == 4 for r in recs)      # a header alone, and three sequence lines
    for b in ref.BINS:
        assert got["pfx.%s.child.fa" % b] == b"".join(r for r, rb in zip(recs, bins[0]) if rb == b), b


def test_malformed_file_and_unknown_reader(inputs, truth):
    d, t = inputs, truth
    recs = [ref.fastq_text([r]) for r in t.trio["r2"]]
    bad = 1000
    lines = recs[bad].split(b"\n")
    recs[bad] = b"\n".join([lines[0], lines[1], b"-", lines[3], b""])
    (d / "bad.fq").write_bytes(b"".join(recs))
    assert sum(map(len, recs[:bad])) > 2 * CHUNK        # the bad record is in a later block: `record 1000` counts the blocks before
    said = {}
    for reader in ("device", "host"):
        before = set(os.listdir(d))
        p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", "R1.fq bad.fq", "--write-reads", "--per-read", "--reader", reader, "-o", "bad"] + PARENTS + THRESHOLDS,
                           cwd=d, env=dict(os.environ, PYTHONPATH=ROOT, **ENV), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1, p.stdout + p.stderr
        said[reader] = [ln.split("] ", 1)[1] for ln in p.stderr.splitlines() if "malformed" in ln]      # (without the time in front)
        assert set(os.listdir(d)) == before
    assert said["device"] == said["host"] == ["bad.fq: record %d is malformed: its third line does not begin with +" % bad]
    # a reader that is none: exit status 1 before a parent is opened (the parents named here do not exist)
    before = set(os.listdir(d))
    p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", "R1.fq", "--mat", "no_such_mat.fa", "--pat", "no_such_pat.fa", "--reader", "x"], cwd=d,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 1 and "--reader takes host or device" in p.stderr and "no_such" not in p.stderr, p.stdout + p.stderr
    assert set(os.listdir(d)) == before
