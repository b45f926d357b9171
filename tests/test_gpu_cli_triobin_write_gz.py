"""GPU: `python -m jasper_amd.triobin --write-reads --write-gz --deflate device` as a child process on the synthetic trio of
test_gpu_cli_triobin.py.  Every bin file's text (through the strict walker, tests/bgzf_ref.py) equals the plain run's file, with the
compressor alone and with every device flag; the tool reads its own .gz output with the device inflater; and a table counted from the
.gz bin files equals one counted from the plain ones."""
import gzip
import os
import re

import pytest

import bgzf_ref
import readbins_ref as ref
from test_gpu_cli_spectra import cli
from test_gpu_cli_triobin import K, PARENTS, THRESHOLDS, Truth

pytestmark = pytest.mark.gpu
CHUNK = 150000
ENV = {"JASPER_TRIOBIN_CHUNK": str(CHUNK), "JASPER_AMD_TIMING": "1"}
ALL_DEVICE = ["--reader", "device", "--gz", "device", "--route", "device"]
FILES = ["R1.fq.gz", "R2.fq"]


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    """the plain run, then --write-gz with the host's compressor, the GPU's alone, and the GPU's under every device flag"""
    d = tmp_path_factory.mktemp("triobin_write_gz")
    t = Truth().trio
    (d / "mat.fa").write_bytes(ref.parent_fasta(t["hap_a"]))
    (d / "pat.fa").write_bytes(ref.parent_fasta(t["hap_b"]))
    (d / "R1.fq.gz").write_bytes(gzip.compress(ref.fastq_text(t["r1"]), 6))
    (d / "R2.fq").write_bytes(ref.fastq_text(t["r2"]))
    args = ["-r", " ".join(FILES), "--paired", "--write-reads"] + PARENTS + THRESHOLDS
    out = {}
    for tag, flags in (("plain", []), ("host", ["--write-gz"]), ("dev", ["--write-gz", "--deflate", "device"]),
                       ("all", ["--write-gz", "--deflate", "device"] + ALL_DEVICE)):
        os.mkdir(d / tag)
        p = cli(d, args + flags + ["-o", tag + "/pfx"], env=ENV, module="jasper_amd.triobin")
        out[tag] = ({fn: open(d / tag / fn, "rb").read() for fn in os.listdir(d / tag)}, p.stderr)
    return d, out


def test_every_bin_file_holds_the_plain_runs_text(runs):
    d, out = runs
    plain = out["plain"][0]
    assert sorted(plain) == sorted(["pfx.readbins.tsv"] + ["pfx.%s.%s" % (b, fn) for b in ref.BINS for fn in ("R1.fq", "R2.fq")])
    assert "[triobin] deflate" not in out["plain"][1]
    for tag in ("host", "dev", "all"):
        files, err = out[tag]
        assert sorted(files) == sorted(fn if fn.endswith(".tsv") else fn + ".gz" for fn in plain), tag
        assert files["pfx.readbins.tsv"].replace(tag.encode() + b"/", b"plain/") == plain["pfx.readbins.tsv"]
        raw = 0
        for fn, data in plain.items():
            if not fn.endswith(".tsv"):
                assert bgzf_ref.walk(files[fn + ".gz"]) == data == gzip.decompress(files[fn + ".gz"]), (tag, fn)
                raw += len(data)
        m = re.search(r"^\[triobin\] deflate (\w+): kernels device seconds (\S+); (\d+) raw bytes, (\d+) compressed bytes; blocks stored (\S+), literal-only (\S+), LZ (\S+)$", err, re.M)
        assert m and m.group(1) == ("host" if tag == "host" else "device") and int(m.group(3)) == raw, err
        assert int(m.group(4)) == sum(len(v) for fn, v in files.items() if fn.endswith(".gz"))
        if tag != "host":                               # the GPU compressed it: its kernels' time and its blocks are on the line
            assert float(m.group(2)) > 0 and int(m.group(5)) + int(m.group(6)) + int(m.group(7)) >= 6
            assert int(m.group(4)) < 0.5 * raw
    assert "[triobin] route kernels device seconds" in out["all"][1]


def test_the_tool_reads_its_own_output_with_the_device_inflater(runs):
    """each bin's two .gz files, R1 and R2, go in again as a pair with every device flag: the templates have the counts they had, so
    every read is binned as before -- the bin's own two files come out whole, the other four are empty -- and the inflater's stats say
    that these multi-member files of the tool's own making were inflated, all of them, in both passes"""
    d, out = runs
    plain = out["plain"][0]
    for b in ref.BINS:
        os.mkdir(d / ("again_" + b))
        files = ["all/pfx.%s.R1.fq.gz" % b, "all/pfx.%s.R2.fq.gz" % b]
        p = cli(d, ["-r", " ".join(files), "--paired", "--write-reads", "-o", "again_%s/pfx" % b] + ALL_DEVICE + PARENTS + THRESHOLDS, env=ENV, module="jasper_amd.triobin")
        for mate in ("R1", "R2"):
            text = plain["pfx.%s.%s.fq" % (b, mate)]
            assert len(text) > 0
            for b2 in ref.BINS:
                got = open(d / ("again_" + b) / ("pfx.%s.pfx.%s.%s.fq" % (b2, b, mate)), "rb").read()
                assert got == (text if b2 == b else b""), (b, mate, b2)
        for second in (False, True):
            pat = r"^\[triobin\] gz stats (\S+)%s: .*\bdevice_bytes=(\d+) host_bytes=(\d+)" % (r" \(second pass\)" if second else "")
            stats = {m.group(1): int(m.group(2)) + int(m.group(3)) for m in re.finditer(pat, p.stderr, re.M)}
            assert stats == {fn: len(plain["pfx.%s.%s.fq" % (b, mate)]) for fn, mate in zip(files, ("R1", "R2"))}, (b, second, p.stderr)
        assert re.search(r"device_bytes=[1-9]", p.stderr)       # and not all of it by the host's zlib behind the inflater


def test_a_table_counted_from_the_gz_bin_files(runs):
    from jasper_amd import KmerTable
    d, out = runs
    hist = []
    for names in (["plain/pfx.mat.R1.fq", "plain/pfx.mat.R2.fq"], ["all/pfx.mat.R1.fq.gz", "all/pfx.mat.R2.fq.gz"], ["dev/pfx.mat.R1.fq.gz", "host/pfx.mat.R2.fq.gz"]):
        t = KmerTable(K, min_slots=1 << 16)
        t.count_files([str(d / fn) for fn in names])
        hist.append(t.histogram())
        t.close()
    assert hist[0] == hist[1] == hist[2] and sum(hist[0]) > 0
