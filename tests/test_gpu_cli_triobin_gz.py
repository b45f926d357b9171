"""GPU: `python -m jasper_amd.triobin --reader device --gz device [--route device]` as a child process on .gz inputs of the synthetic
trio of test_gpu_cli_triobin.py.  Every output file equals, byte for byte, what the same command writes with --reader host, and the
table equals what that module's Truth builds from the restatement and the rule.  That the text really was inflated on the GPU is read
off the inflater's stats line: device_bytes is the decompressed length, which no run without the device inflater can print."""
import gzip
import os
import re
import subprocess
import sys

import pytest

import readbins_ref as ref
from test_gpu_cli_spectra import ROOT, cli
from test_gpu_cli_triobin import PARENTS, THRESHOLDS, Truth
from test_gpu_cli_triobin_reader import fasta_records

pytestmark = pytest.mark.gpu
CHUNK = 150000                  # the files hold 240 to 490 kB of text: several chunks each, their ends inside records
ENV = {"JASPER_TRIOBIN_CHUNK": str(CHUNK), "JASPER_AMD_TIMING": "1"}
MODES = {"host": ["--reader", "host"], "gz": ["--reader", "device", "--gz", "device"], "gz_route": ["--reader", "device", "--gz", "device", "--route", "device"]}


@pytest.fixture(scope="module")
def truth():
    return Truth()


def members(data, n):
    cuts = [len(data) * i // n for i in range(n + 1)]
    return b"".join(gzip.compress(data[a:b]) for a, b in zip(cuts, cuts[1:]))


@pytest.fixture(scope="module")
def inputs(hip, truth, tmp_path_factory):
    d = tmp_path_factory.mktemp("triobin_gz")
    t = truth.trio
    (d / "mat.fa").write_bytes(ref.parent_fasta(t["hap_a"]))
    (d / "pat.fa").write_bytes(ref.parent_fasta(t["hap_b"]))
    text = {"R1.fq.gz": ref.fastq_text(t["r1"]), "R2.fq.gz": ref.fastq_text(t["r2"]), "multi_R1.fastq.gz": ref.fastq_text(t["r1"]),
            "multi_R2.fastq.gz": ref.fastq_text(t["r2"], b"\r\n"), "child.fa.gz": b"".join(fasta_records(t["r2"]))}
    for fn, data in text.items():
        (d / fn).write_bytes(members(data, 4) if fn.startswith("multi") else gzip.compress(data, 6))
        assert len(data) > 1.5 * CHUNK
    return d, text


def run_modes(d, args, tag):
    """the command in every mode, each into its own directory -> {mode: ({file: bytes}, stderr)}"""
    got = {}
    for mode, flags in MODES.items():
        os.mkdir(d / (tag + mode))
        p = cli(d, args + flags + ["-o", "%s%s/pfx" % (tag, mode)] + PARENTS + THRESHOLDS, env=ENV, module="jasper_amd.triobin")
        got[mode] = ({fn: open(d / (tag + mode) / fn, "rb").read() for fn in os.listdir(d / (tag + mode))}, p.stderr)
    return got


def device_bytes(stderr, second_pass=False):
    """{file: device_bytes} of the inflater's stats lines"""
    pat = r"^\[triobin\] gz stats (\S+)%s: .*\bdevice_bytes=(\d+) host_bytes=(\d+)" % (r" \(second pass\)" if second_pass else "")
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(pat, stderr, re.M)}


def check_modes(got, text, files, n_outputs):
    host = got["host"][0]
    assert len(host) == n_outputs and not any(fn.endswith(".tmp") for fn in host)
    for mode in ("gz", "gz_route"):
        assert got[mode][0] == host, mode
        err = got[mode][1]
        assert device_bytes(err) == {fn: (len(text[fn]), 0) for fn in files}, mode      # inflated on the GPU, all of it
        assert "[triobin] gz inflate seconds by events" in err and "[triobin] second pass wall seconds" in err
        assert ("[triobin] route kernels device seconds" in err) == (mode == "gz_route")
        assert device_bytes(err, second_pass=True) == ({fn: (len(text[fn]), 0) for fn in files} if mode == "gz_route" else {})
    assert "gz stats" not in got["host"][1]


def test_pairs_and_members(inputs, truth):
    d, text = inputs
    files = ["R1.fq.gz", "R2.fq.gz", "multi_R1.fastq.gz", "multi_R2.fastq.gz"]
    got = run_modes(d, ["-r", " ".join(files), "--paired", "--per-read", "--write-reads"], "a_")
    check_modes(got, text, files, 2 + 3 * 4)
    want_tsv, want_reads, bins = truth.files(files, ["r1", "r2", "r1", "r2"], paired=True)
    out = got["gz_route"][0]
    assert out["pfx.readbins.tsv"].decode() == want_tsv and out["pfx.readbins.reads.tsv"].decode() == want_reads
    for fn, fb in zip(files, bins):                     # each input's three files hold each of its records once, in its bin
        eol = b"\r\n" if fn == "multi_R2.fastq.gz" else b"\n"
        recs = [b"".join(ln + eol for ln in rec) for rec in zip(*[iter(text[fn].split(eol)[:-1])] * 4)]
        for b in ref.BINS:
            assert out["pfx.%s.%s" % (b, fn[:-3])] == b"".join(r for r, rb in zip(recs, fb) if rb == b), (fn, b)


def test_fasta(inputs, truth):
    d, text = inputs
    got = run_modes(d, ["-r", "child.fa.gz", "--per-read", "--write-reads"], "b_")
    check_modes(got, text, ["child.fa.gz"], 2 + 3)
    want_tsv, want_reads, bins = truth.files(["child.fa.gz"], ["r2"])
    out = got["gz_route"][0]
    assert out["pfx.readbins.tsv"].decode() == want_tsv and out["pfx.readbins.reads.tsv"].decode() == want_reads
    recs = fasta_records(truth.trio["r2"])
    for b in ref.BINS:
        assert out["pfx.%s.child.fa" % b] == b"".join(r for r, rb in zip(recs, bins[0]) if rb == b), b


def test_corrupt_gz_ends_the_run(inputs):
    d, text = inputs
    blob = bytearray((d / "R2.fq.gz").read_bytes())
    blob[-8] ^= 0x55                                    # the CRC-32 of the trailer
    (d / "crc.fq.gz").write_bytes(bytes(blob))
    (d / "cut.fq.gz").write_bytes((d / "R2.fq.gz").read_bytes()[:-3000])
    for bad in ("crc.fq.gz", "cut.fq.gz"):
        before = set(os.listdir(d))
        p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", "R1.fq.gz " + bad, "--write-reads", "--per-read", "-o", "bad"] + MODES["gz_route"] + PARENTS +
                           THRESHOLDS, cwd=d, env=dict(os.environ, PYTHONPATH=ROOT, **ENV), capture_output=True, text=True, timeout=600)
        assert p.returncode == 1, p.stdout + p.stderr
        said = [ln for ln in p.stderr.splitlines() if "cannot be inflated" in ln]
        assert len(said) == 1 and bad in said[0] and "Traceback" not in p.stderr, p.stderr
        assert set(os.listdir(d)) == before


HOOK = """
import os, sys
from jasper_amd import triobin
second = triobin._write_reads_by_starts
def swap(paths, *a, **k):
    os.replace(sys.argv[1], paths[0])                   # between the two passes: another file under the name
    return second(paths, *a, **k)
triobin._write_reads_by_starts = swap
sys.exit(triobin.run(sys.argv[2:]))
"""


def test_file_changed_between_the_passes(inputs):
    d, text = inputs
    data = text["R2.fq.gz"]
    shifted = data.replace(b"@", b"@x", 1)[:len(data)]  # the same length, every later record one byte further on
    for name, changed, modes in (("longer", data + data[:data.index(b"@", 1)], ("gz_route",)), ("shorter", data[:-9], ("gz_route",)), ("shifted", shifted, ("gz", "gz_route"))):
        for mode in modes:
            (d / "victim.fq.gz").write_bytes(gzip.compress(data))
            (d / "next.gz").write_bytes(gzip.compress(changed))
            before = set(os.listdir(d)) - {"next.gz"}
            p = subprocess.run([sys.executable, "-c", HOOK, "next.gz", "-r", "victim.fq.gz", "--write-reads", "-o", "chg"] + MODES[mode] + PARENTS + THRESHOLDS, cwd=d,
                               env=dict(os.environ, PYTHONPATH=ROOT, **ENV), capture_output=True, text=True, timeout=600)
            assert p.returncode == 1 and "--write-reads: victim.fq.gz changed between the two passes" in p.stderr, (name, mode, p.stdout + p.stderr)
            assert set(os.listdir(d)) == before, (name, mode)
