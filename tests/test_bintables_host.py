"""CPU: the host side of `triobin --write-jf` -- the identity it rests on, restated on Counters of canonical k-mer strings; the flag and its
checks; the counting pass and the writer with the GPU calls replaced by the restatement (the tool's _WriteJf reaches the GPU only through
KmerTable, which is swapped for a table of Counters here); and csrc/bincount_plan.hpp built and run as a stand-alone program under
-fsanitize=address,undefined (tools/bincount_plan_check.cpp).  The GPU tests (test_gpu_count_binned.py, test_gpu_subtract.py,
test_gpu_cli_triobin_write_jf.py) put the kernels there."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

import layout_util as lu
import markers_ref as mr
import readbins_ref as ref
import test_triobin_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def bin_counters(reads, bins, k, names):
    """reads = per input [(name, sequence)], bins = per input the bin names -> {bin: Counter of its reads' canonical k-mers}"""
    per = {b: collections.Counter() for b in names}
    for fr, fb in zip(reads, bins):
        for (_, s), b in zip(fr, fb):
            per[b].update(lu.kmer_counter(s, k))
    return per


def minus(r, t):
    """R - T key by key -> (the difference without its zeros, dropped, reduced, unchanged keys); T must be a sub-multiset"""
    assert all(r[km] >= c for km, c in t.items())
    d = {km: c - t.get(km, 0) for km, c in r.items() if c > t.get(km, 0)}
    return d, len(r) - len(d), sum(1 for km, c in d.items() if c < r[km]), sum(1 for km, c in d.items() if c == r[km])


def test_identity_on_an_example_worked_by_hand():
    k = 5
    reads = [[("a", b"AACCGTT"), ("b", b"AACCG"), ("c", b"ttaaccgNAACCG"), ("d", b"AACC")]]
    per = bin_counters(reads, [["mat", "pat", "unknown", "mat"]], k, ref.BINS)
    assert per["mat"] == {"AACCG": 1, "ACCGT": 1, "AACGG": 1} and per["pat"] == {"AACCG": 1}          # (AACGG: CCGTT's reverse complement)
    assert per["unknown"] == {"AACCG": 2, "GTTAA": 1, "GGTTA": 1}                                     # (lower case counts, N cuts; TTAAC and TAACC by their reverse complements)
    everything = per["mat"] + per["pat"] + per["unknown"]
    d, dropped, reduced, unchanged = minus(everything, per["pat"])
    assert d == dict(per["mat"] + per["unknown"]) and d["AACCG"] == 3 and (dropped, reduced, unchanged) == (0, 1, 4)
    d, dropped, reduced, unchanged = minus(everything, per["mat"])
    assert d == dict(per["pat"] + per["unknown"]) and (dropped, reduced, unchanged) == (2, 1, 2)


def test_haps_fixture_is_no_vacuous_input():
    """asserted on the restatement alone, before any GPU comparison: every bin holds reads, single-ended and paired, and R - T2 drops
    keys (k-mers only hap2's reads hold), reduces keys (shared with hap1's or unknown reads) and leaves keys unchanged"""
    h = mr.make_haps()
    k = ref.TRIO_K
    reads = {"r1": h["r1"], "r2": h["r2"]}
    t = mr.Haps(k, [h["hap1"]], [h["hap2"]], reads, "solid", mr.HAPS_THRE)
    numbers = []
    for paired in (False, True):
        _, _, bins = t.files(["R1.fq", "R2.fq"], ["r1", "r2"], paired=paired)
        flat = bins[0] + bins[1]
        numbers += [flat.count(b) for b in mr.BINS]
        if not paired:
            per = bin_counters([h["r1"], h["r2"]], bins, k, mr.BINS)
            everything = per["hap1"] + per["hap2"] + per["unknown"]
            for own, other in (("hap1", "hap2"), ("hap2", "hap1")):
                d, dropped, reduced, unchanged = minus(everything, per[other])
                assert d == dict(per[own] + per["unknown"])
                if own == "hap1":
                    numbers += [dropped, reduced, unchanged]
                assert min(dropped, reduced, unchanged) > 100
    assert len(numbers) == 9 and min(numbers) > 100, numbers


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def test_the_flag_and_its_checks(tmp_path, capsys, monkeypatch):
    from jasper_amd import triobin
    assert triobin.parse_args(["-r", "x.fq"])["write_jf"] is False
    a = triobin.parse_args(["-r", "x.fq", "--write-jf", "--write-reads"])
    assert a["write_jf"] is True and a["write_reads"] is True
    assert "--write-jf" in triobin.USAGE and "--write-jf" in triobin.__doc__
    for fn in ("R1.fq", "R2.fq", "mat.fq", "pat.fq", "hap1.fa", "hap2.fa"):
        (tmp_path / fn).write_bytes(ref.fastq_text(th.READS) if fn.endswith(".fq") else b">c\nACGTACGTTT\n" + fn.encode()[:4].upper().replace(b"H", b"A").replace(b"P", b"C") + b"\n")
    th.fake_jf(tmp_path / "p.hap2.jf", 21)
    th.fake_jf(tmp_path / "child.jf", 21)
    monkeypatch.chdir(tmp_path)
    # usable in both modes, with or without --write-reads, with every reader
    for argv in (["-r", "R1.fq", "--write-jf", "--mat", "mat.fq", "--pat", "pat.fq"],
                 ["-r", "R1.fq R2.fq", "--write-jf", "--paired", "--reader", "device", "--gz", "device", "--hap1", "hap1.fa", "--hap2", "hap2.fa", "--child-jf", "child.jf"]):
        a = triobin.parse_args(argv)
        reader = triobin.check_reader(a)
        triobin.check_gz_route(a, reader)
        triobin.check_write_gz(a)
        reads, k, device, hap, _, _ = triobin.check_flags(a)
        triobin.check_write_jf(a, hap, "p", triobin.HAP_BINS if "hap1" in hap else triobin.BINS)
    # a database it would write is the one --child-jf reads: refused before anything is opened
    monkeypatch.setattr("jasper_amd.triobin.open_haps", lambda *a, **k: pytest.fail("a table was opened"))
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        triobin.run(["-r", "R1.fq", "--write-jf", "-o", "p", "--hap1", "hap1.fa", "--hap2", "hap2.fa", "--child-jf", "./p.hap2.jf"])
    assert e.value.code == 1 and "p.hap2.jf would be written over the --child-jf database" in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == before


# ---- the pass and the writer, on Counters ---------------------------------------------------------------------------------------------
class FakeTable:
    """what _WriteJf uses of KmerTable, on a Counter of canonical k-mer strings"""
    calls = []

    def __init__(self, k, min_slots=0, device=0):
        self.k, self.c, self.open = k, collections.Counter(), True

    @staticmethod
    def count_binned(reads, codes, sinks):
        text, offs = reads
        assert text.dtype == np.uint8 and offs.dtype == np.int64 and offs[0] == 0 and offs[-1] == len(text) and len(codes) == len(offs) - 1
        FakeTable.calls.append(len(codes))
        seqs = ref.split(text.tobytes(), offs.tolist())
        out = []
        for t, bins in sinks:
            assert t.open
            mine = [s for s, c in zip(seqs, codes.tolist()) if c in bins]
            add = lu.kmer_counter(b"\n".join(mine), t.k)
            t.c.update(add)
            out.append(dict(reads=len(mine), bases=sum(len(s) for s in mine), occurrences=sum(add.values()), gather_seconds=0.0, count_seconds=0.0))
        return out

    @staticmethod
    def subtract(src, minus_):
        assert src.open and minus_.open
        dst = FakeTable(src.k)
        dst.c = collections.Counter({km: c - minus_.c.get(km, 0) for km, c in src.c.items() if c > minus_.c.get(km, 0)})
        under = sum(1 for km, c in src.c.items() if minus_.c.get(km, 0) > c)
        matched = sum(1 for km in src.c if km in minus_.c)
        return dst, dict(swept=len(src.c), matched=matched, dropped=len(src.c) - len(dst.c) - under, underflow=under, kept=len(dst.c), missing=len(minus_.c) - matched,
                         seconds=0.0)

    def write_jf(self, path, cmdline=()):
        assert self.open and path.endswith(".jf.tmp")
        with open(path, "w") as f:
            f.write(" ".join(cmdline) + "\n" + "".join("%s %d\n" % kv for kv in sorted(self.c.items())))

    def info(self):
        return dict(k=self.k, distinct=len(self.c), occurrences=sum(self.c.values()))

    def close(self):
        self.open = False


def read_fake(path):
    lines = open(path).read().splitlines()
    return lines[0], {ln.split()[0]: int(ln.split()[1]) for ln in lines[1:]}


@pytest.mark.parametrize("keep_r", [False, True])
def test_the_pass_gives_each_sink_its_reads_and_the_files_hold_the_differences(tmp_path, monkeypatch, keep_r):
    """on the hand-made reads of test_triobin_host in every format the reader takes, the parser's block cutting every record: T1 and T2
    get their bins' reads, R all of them (a third sink) or none (R kept), and the two files hold R - T2 and R - T1"""
    from jasper_amd import triobin
    files = th.write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    _, _, bins = th.expected(paths)
    per = bin_counters([th.READS] * len(paths), bins, th.K, ref.BINS)
    everything = per["mat"] + per["pat"] + per["unknown"]
    assert per["mat"] and per["pat"] and per["unknown"]
    monkeypatch.setattr(triobin, "KmerTable", FakeTable)
    monkeypatch.setattr(triobin, "CHUNK", 64)
    FakeTable.calls = []
    kept = None
    if keep_r:
        kept = FakeTable(th.K)
        kept.c = collections.Counter(everything)
    prefix = str(tmp_path / "out")
    jf = triobin._WriteJf(None, kept, th.K, 0, prefix, triobin.BINS, paths, "host", None)
    per_bin, _ = triobin.bin_files(paths, prefix, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, write_jf=jf)
    assert len(FakeTable.calls) > len(paths) and sum(FakeTable.calls) == len(paths) * len(th.READS)
    for own, other in (("mat", "pat"), ("pat", "mat")):
        head, got = read_fake("%s.%s.jf" % (prefix, own))
        assert got == minus(everything, per[other])[0] == dict(per[own] + per["unknown"])
        assert head == "count -C -m %d -o %s.%s.jf %s" % (th.K, prefix, own, " ".join(paths))
    assert [d[:2] for d in jf.databases] == [(prefix + ".mat.jf", ("mat", "unknown")), (prefix + ".pat.jf", ("pat", "unknown"))]
    assert [d[2:] for d in jf.databases] == [(len(per[b] + per["unknown"]), sum((per[b] + per["unknown"]).values())) for b in ("mat", "pat")]
    assert [s["reads"] for s in jf.timing["sums"]] == [per_bin[0][0], per_bin[1][0]] + ([] if keep_r else [sum(r for r, _ in per_bin)])
    assert kept is None or kept.open                    # a kept table is the caller's to close
    assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]


def test_a_failed_run_leaves_no_database(tmp_path, monkeypatch, capsys):
    """a reads' table that is not these reads' (here: one that lacks a k-mer of the paternal reads) ends the run with exit status 1 and
    its message after the first database was written as .tmp; a file that changes between the passes ends it with --write-reads' wording.
    Neither leaves a file"""
    from jasper_amd import triobin
    (tmp_path / "a.fq").write_bytes(ref.fastq_text(th.READS))
    paths = [str(tmp_path / "a.fq")]
    _, _, bins = th.expected(paths)
    per = bin_counters([th.READS], bins, th.K, ref.BINS)
    monkeypatch.setattr(triobin, "KmerTable", FakeTable)
    wrong = FakeTable(th.K)
    wrong.c = per["mat"] + per["unknown"]
    before = sorted(os.listdir(tmp_path))
    jf = triobin._WriteJf(None, wrong, th.K, 0, str(tmp_path / "out"), triobin.BINS, paths, "host", None)
    with pytest.raises(SystemExit) as e:
        triobin.bin_files(paths, str(tmp_path / "out"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, write_jf=jf)
    assert e.value.code == 1 and "--child-jf is not the database of these reads" in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == before

    real_chunks = triobin.chunks
    passes = []

    def chunks(path, want_seq=True):
        passes.append(path)
        if len(passes) == 3:                            # (the first pass, --write-reads' pass, then --write-jf's)
            with open(path, "ab") as f:
                f.write(ref.fastq_text(th.READS[:1]))
        return real_chunks(path, want_seq)

    monkeypatch.setattr(triobin, "chunks", chunks)
    jf = triobin._WriteJf(None, None, th.K, 0, str(tmp_path / "out"), triobin.BINS, paths, "host", None)
    with pytest.raises(SystemExit) as e:
        triobin.bin_files(paths, str(tmp_path / "out"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, write_jf=jf)
    assert e.value.code == 1 and "--write-jf: %s changed between the two passes" % paths[0] in capsys.readouterr().err
    assert sorted(os.listdir(tmp_path)) == before


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_bincount_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path / "bincount_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bincount_plan_check.cpp"), "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    assert int(p.stdout.split()[1]) > 500
