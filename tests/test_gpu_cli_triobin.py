"""GPU: `python -m jasper_amd.triobin` as a child process on a 20 kb synthetic trio (tests/readbins_ref.py: make_trio).  Every file it
writes equals, byte for byte, what the restatement and the rule give from Python dicts of the parents' k-mers; nothing expected here comes
from the code under test.  That the trio is no vacuous input -- at least 90 % of the reads binned, some left unknown -- is asserted on the
restatement alone in test_triobin_host.py, and once more here before anything is compared."""
import gzip
import os
import subprocess
import sys

import pytest

import readbins_ref as ref
from test_gpu_cli_spectra import ROOT, cli, messages

pytestmark = pytest.mark.gpu
K = ref.TRIO_K
THRE = 2
PARENTS = ["--mat", "mat.fa", "--pat", "pat.fa", "-k", str(K)]
THRESHOLDS = ["--mat-threshold", str(THRE), "--pat-threshold", str(THRE)]


class Truth:
    """the trio, its files' records and what every output holds for a list of input files"""

    def __init__(self):
        t = ref.make_trio()
        self.trio = t
        self.md, self.pd = ref.kmer_dict([t["hap_a"]], K, 4), ref.kmer_dict([t["hap_b"]], K, 4)
        self.m_total, self.p_total = ref.hapmer_total(self.md, self.pd, THRE), ref.hapmer_total(self.pd, self.md, THRE)
        self.counts = {f: ref.read_counts([s for _, s in t[f]], K, self.md, self.pd, THRE, THRE) for f in ("r1", "r2")}

    def write(self, d):
        t = self.trio
        (d / "mat.fa").write_bytes(ref.parent_fasta(t["hap_a"]))
        (d / "pat.fa").write_bytes(ref.parent_fasta(t["hap_b"]))
        (d / "R1.fq").write_bytes(ref.fastq_text(t["r1"]))
        (d / "R2.fq").write_bytes(ref.fastq_text(t["r2"]))
        os.mkdir(d / "z")
        with gzip.open(d / "z" / "R1.fastq.gz", "wb") as f:
            f.write(ref.fastq_text(t["r1"]))
        (d / "z" / "R2_crlf.fastq").write_bytes(ref.fastq_text(t["r2"], b"\r\n"))
        (d / "short.fq").write_bytes(ref.fastq_text(t["r2"][:-3]))

    def files(self, paths, which, paired=False, min_markers=1):
        """paths: the inputs as given, which: "r1" / "r2" for each -> (readbins.tsv, reads.tsv, per input its bins)"""
        reads = [self.trio[w] for w in which]
        lens = [[len(s) for _, s in r] for r in reads]
        names = [[n for n, _ in r] for r in reads]
        ms, ps = [self.counts[w][0] for w in which], [self.counts[w][1] for w in which]
        bins = ref.file_bins(ms, ps, self.m_total, self.p_total, min_markers, paired)
        return ref.readbins_tsv(paths, lens, ms, ps, bins), ref.per_read_tsv(paths, names, lens, ms, ps, bins), bins


@pytest.fixture(scope="module")
def truth():
    return Truth()


@pytest.fixture(scope="module")
def inputs(hip, truth, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin")
    truth.write(d)
    return d


def check_read_files(d, prefix, base, data, eol, bins):
    recs = [b"".join(ln + eol for ln in rec) for rec in zip(*[iter(data.split(eol)[:-1])] * 4)]
    assert len(recs) == len(bins)
    for b in ref.BINS:
        assert open(d / ("%s.%s.%s" % (prefix, b, base)), "rb").read() == b"".join(r for r, rb in zip(recs, bins) if rb == b), (base, b)


def test_files_equal_the_restatement(inputs, truth):
    d, t = inputs, truth
    want_tsv, want_reads, bins = t.files(["R1.fq", "R2.fq"], ["r1", "r2"])
    flat = bins[0] + bins[1]
    assert flat.count("mat") + flat.count("pat") >= 0.9 * len(flat) and flat.count("unknown") >= 1      # first: no vacuous input
    before = set(os.listdir(d))
    p = cli(d, ["-r", "R1.fq R2.fq", "--per-read", "--write-reads"] + PARENTS + THRESHOLDS, env={"JASPER_AMD_TIMING": "1"}, module="jasper_amd.triobin")
    made = sorted(set(os.listdir(d)) - before)
    assert made == sorted(["R1.fq.readbins.tsv", "R1.fq.readbins.reads.tsv"] + ["R1.fq.%s.%s" % (b, f) for b in ref.BINS for f in ("R1.fq", "R2.fq")])      # (PREFIX: the first read file)
    assert open(d / "R1.fq.readbins.tsv").read() == want_tsv
    assert open(d / "R1.fq.readbins.reads.tsv").read() == want_reads
    for f, w, fb in (("R1.fq", "r1", bins[0]), ("R2.fq", "r2", bins[1])):
        check_read_files(d, "R1.fq", f, ref.fastq_text(t.trio[w]), b"\n", fb)
    log = messages(p.stdout)
    assert len(log) == 2 and "k = %d" % K in log[0] and "maternal threshold %d (given)" % THRE in log[0]
    assert "%d maternal and %d paternal hap-mers" % (t.m_total, t.p_total) in log[0]
    assert "mat %d reads" % flat.count("mat") in log[1] and "unknown %d reads" % flat.count("unknown") in log[1]
    assert "[triobin] read_bins device seconds" in p.stderr
    for fn in made:
        os.remove(d / fn)


def test_pairs_gz_crlf_and_small_batches(inputs, truth):
    """--paired with R1 as .gz and R2 with CRLF line ends, --batch-bases 300 (two reads of 150 bases a batch), --min-markers 2, -o"""
    d, t = inputs, truth
    paths = ["z/R1.fastq.gz", "z/R2_crlf.fastq"]
    want_tsv, want_reads, bins = t.files(paths, ["r1", "r2"], paired=True, min_markers=2)
    assert bins[0] == bins[1] and bins[0] != t.files(paths, ["r1", "r2"])[2][0]      # the pairs' sums decide otherwise than the reads alone
    os.mkdir(d / "out")
    before = set(os.listdir(d))
    cli(d, ["-r", " ".join(paths), "--paired", "--per-read", "--write-reads", "--batch-bases", "300", "--min-markers", "2", "-o", "out/pfx"] + PARENTS + THRESHOLDS,
        module="jasper_amd.triobin")
    assert set(os.listdir(d)) == before
    assert sorted(os.listdir(d / "out")) == sorted(["pfx.readbins.tsv", "pfx.readbins.reads.tsv"] + ["pfx.%s.%s" % (b, f) for b in ref.BINS for f in ("R1.fastq", "R2_crlf.fastq")])
    assert open(d / "out" / "pfx.readbins.tsv").read() == want_tsv
    assert open(d / "out" / "pfx.readbins.reads.tsv").read() == want_reads
    check_read_files(d / "out", "pfx", "R1.fastq", ref.fastq_text(t.trio["r1"]), b"\n", bins[0])
    check_read_files(d / "out", "pfx", "R2_crlf.fastq", ref.fastq_text(t.trio["r2"], b"\r\n"), b"\r\n", bins[1])


def test_errors_leave_no_files(inputs):
    d = inputs
    for args, message in ((["-r", "R1.fq short.fq", "--paired", "--write-reads", "--per-read"] + PARENTS + THRESHOLDS, "the files of a pair must hold the same templates"),
                          (["-r", "R1.fq"] + PARENTS, "k-mer histogram gives no threshold")):      # every k-mer of a parent occurs four times: no descent to follow
        before = set(os.listdir(d))
        p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin"] + args, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1 and message in p.stderr, p.stdout + p.stderr
        assert set(os.listdir(d)) == before
