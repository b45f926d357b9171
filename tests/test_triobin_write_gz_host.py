"""CPU: `python -m jasper_amd.triobin --write-reads --write-gz [--deflate host]` -- the flags, the BGZF bin files of the host compressor
against the plain files of the same run, and the plan header of the GPU compressor under a sanitizer.  The GPU's parts are stand-ins as
in test_triobin_gz_host.py; tests/test_gpu_cli_triobin_write_gz.py runs the real ones."""
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import bgzf_ref
import readbins_ref as ref
import readroute_ref as rr
import test_triobin_host as th
from test_triobin_gz_host import FakeSession
from test_triobin_reader_host import fake_count_text, never

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_are_checked_before_a_parent_is_opened(tmp_path, capsys, monkeypatch):
    from jasper_amd import triobin
    for fn in ("R1.fq", "mat.fq", "pat.fq"):
        (tmp_path / fn).write_bytes(ref.fastq_text(th.READS))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("jasper_amd.extensions.open_parents", lambda *a, **k: pytest.fail("a parent was opened"))
    base = ["-r", "R1.fq", "--mat", "mat.fq", "--pat", "pat.fq"]
    cases = [
        (["--write-gz"], "--write-gz needs --write-reads"),
        (["--write-gz", "--deflate", "device"], "--write-gz needs --write-reads"),
        (["--write-reads", "--deflate", "host"], "--deflate host needs --write-gz"),
        (["--write-reads", "--deflate", "device"], "--deflate device needs --write-gz"),
        (["--deflate", "device"], "--deflate device needs --write-gz"),
        (["--write-reads", "--write-gz", "--deflate", "gpu"], "--deflate takes host or device; gpu was given"),
        (["--deflate", "zlib"], "--deflate takes host or device; zlib was given"),
        (["--write-reads", "--write-gz", "--deflate"], "Unknown option --deflate"),
    ]
    before = sorted(os.listdir(tmp_path))
    for extra, message in cases:
        with pytest.raises(SystemExit) as e:
            triobin.run(base + extra)
        assert e.value.code == 1, extra
        out = capsys.readouterr()
        assert message in out.err + out.out, extra
        assert sorted(os.listdir(tmp_path)) == before, extra
    assert triobin.check_write_gz(triobin.parse_args(base)) == (False, "host")
    assert triobin.check_write_gz(triobin.parse_args(base + ["--write-reads", "--write-gz"])) == (True, "host")
    assert triobin.check_write_gz(triobin.parse_args(base + ["--write-reads", "--write-gz", "--deflate", "device"])) == (True, "device")
    assert "--write-gz" in triobin.USAGE and "--deflate host|device" in triobin.USAGE


def bin_texts(tmp_path, prefix, files, gz):
    """{(bin, input): the bin file's text}; with gz through the walker, and gzip must read the same"""
    out = {}
    for fn in files:
        base = fn[:-3] if fn.endswith(".gz") else fn
        for b in ref.BINS:
            name = "%s.%s.%s%s" % (prefix, b, base, ".gz" if gz else "")
            blob = open(name, "rb").read()
            if gz:
                assert not os.path.exists(name[:-3]), name      # no plain file beside it
                assert gzip.decompress(blob) == bgzf_ref.walk(blob)
            out[(b, fn)] = bgzf_ref.walk(blob) if gz else blob
    return out


@pytest.mark.parametrize("chunk", [16 << 20, 64, 7])
def test_host_reader_bin_files_hold_the_plain_files_text(tmp_path, monkeypatch, chunk):
    from jasper_amd import triobin
    files = th.write_formats(tmp_path)                          # FASTQ and FASTA, LF and CRLF, .gz inputs, files without a last line end
    paths = [str(tmp_path / fn) for fn in files]
    monkeypatch.setattr(triobin, "CHUNK", chunk)                # (blocks that cut every record: every write is members of its own)
    plain, packed = str(tmp_path / "plain"), str(tmp_path / "packed")
    per_plain, _ = triobin.bin_files(paths, plain, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True)
    timings = {}
    per_gz, _ = triobin.bin_files(paths, packed, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True, write_gz=True, timings=timings)
    assert per_gz == per_plain
    want, got = bin_texts(tmp_path, plain, files, False), bin_texts(tmp_path, packed, files, True)
    assert got == want
    assert sum(len(v) for v in want.values()) == sum(len(d) for d in files.values()) == timings["deflate_raw"]
    assert timings["deflate_written"] == sum(os.path.getsize("%s.%s.%s.gz" % (packed, b, fn[:-3] if fn.endswith(".gz") else fn)) for b in ref.BINS for fn in files)
    for tail in (".readbins.tsv", ".readbins.reads.tsv"):
        assert open(packed + tail).read().replace(packed, plain) == open(plain + tail).read()
    assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]


def test_a_bin_that_stays_empty_is_the_end_marker_alone(tmp_path):
    from jasper_amd import triobin
    path = tmp_path / "only.fq"
    path.write_bytes(ref.fastq_text(th.READS[:1]))              # r0 alone: maternal
    triobin.bin_files([str(path)], str(tmp_path / "o"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, write_gz=True)
    assert bgzf_ref.walk(open(tmp_path / "o.mat.only.fq.gz", "rb").read()) == ref.fastq_text(th.READS[:1])
    for b in ("pat", "unknown"):
        blob = open(tmp_path / ("o.%s.only.fq.gz" % b), "rb").read()
        assert blob == bgzf_ref.EOF_MARKER and len(blob) == 28


def test_paired_files_stay_in_step(tmp_path):
    from jasper_amd import triobin
    th.write_formats(tmp_path)
    paths = [str(tmp_path / "a.fq"), str(tmp_path / "f.fq.gz")]
    triobin.bin_files(paths, str(tmp_path / "pp"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, paired=True, write_reads=True)
    triobin.bin_files(paths, str(tmp_path / "pg"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, paired=True, write_reads=True, write_gz=True)
    for b in ref.BINS:
        texts = [bgzf_ref.walk(open(tmp_path / ("pg.%s.%s.gz" % (b, base)), "rb").read()) for base in ("a.fq", "f.fq")]
        assert texts == [open(tmp_path / ("pp.%s.%s" % (b, base)), "rb").read() for base in ("a.fq", "f.fq")]
        assert texts[0] == texts[1]                             # the two files hold the same reads: the mates went to the same bin


def fake_route_text_gz(log):
    """what KmerTable.route_text gives with and without gz=True: the restatement's bytes, compressed by the host's compressor"""
    from jasper_amd import bgzf

    def route_text(buf, bounds, bins, first, check_from, out, gz=False):
        outs, bad = rr.route(buf.tobytes(), bounds, bins, first[0], check_from)
        log.append(gz)
        if not gz:
            return types.SimpleNamespace(out=[np.frombuffer(o, dtype=np.uint8) for o in outs], mismatches=bad, seconds=0.0)
        assert all(len(o) >= len(buf) + 31 * -(-len(buf) // 65280) for o in out)        # room for the bound
        return types.SimpleNamespace(out=[np.frombuffer(bgzf.compress(o), dtype=np.uint8) for o in outs], mismatches=bad, seconds=0.0, raw_bytes=[len(o) for o in outs],
                                     deflate={"stored": 0, "literal_only": 0, "lz": sum(1 for o in outs if o)}, deflate_seconds=0.25)
    return route_text


class FakeSessionGz(FakeSession):
    def route(self, want, bounds, bins, first, check_from, out, gz=False):
        from jasper_amd import bgzf
        r = FakeSession.route(self, want, bounds, bins, first, check_from, out)
        if gz and r.routed:
            r.raw_bytes = [len(o) for o in r.out]
            r.out = [np.frombuffer(bgzf.compress(o), dtype=np.uint8) for o in r.out]
            r.deflate, r.deflate_seconds = {"stored": 0, "literal_only": 0, "lz": 1}, 0.25
        return r


@pytest.mark.parametrize("chunk", [None, 9])
def test_device_reader_and_every_deflate_path_write_the_same_text(tmp_path, monkeypatch, chunk):
    """--reader device with the four writers: plain, host BGZF, a device compressor per write, members from the route calls"""
    from jasper_amd import bgzf, triobin
    files = th.write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    if chunk is not None:
        monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", str(chunk))
        monkeypatch.setattr(triobin, "CHUNK", 5 * chunk + 3)
    plain = str(tmp_path / "plain")
    triobin.bin_files(paths, plain, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True)
    want = bin_texts(tmp_path, plain, files, False)
    calls = []

    def deflate(arr):
        assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and len(arr)
        calls.append(len(arr))
        return np.frombuffer(bgzf.compress(arr), dtype=np.uint8), {"stored": 1, "literal_only": 2, "lz": 3}, 0.5

    for name, kw in (("h", {}), ("d", dict(deflate=deflate)), ("r", dict(deflate=deflate, route=True)), ("rh", dict(route=True))):
        log, timings, n_calls = [], {}, len(calls)
        route = kw.pop("route", False)
        prefix = str(tmp_path / name)
        triobin.bin_files(paths, prefix, never, th.M_TOTAL, th.P_TOTAL, write_reads=True, reader="device", count_text=fake_count_text(),
                          gz_open=(lambda p: FakeSessionGz(p, [])) if route else None, route_text=fake_route_text_gz(log) if route else None, write_gz=True,
                          timings=timings, **kw)
        assert bin_texts(tmp_path, prefix, files, True) == want, name
        assert timings["deflate_raw"] == sum(len(d) for d in files.values())
        if name == "d":
            assert len(calls) > n_calls and timings["deflate_blocks"] == {"stored": len(calls), "literal_only": 2 * len(calls), "lz": 3 * len(calls)}
            assert timings["deflate_seconds"] == 0.5 * len(calls)
        if name == "r":                                         # the route calls compress: the per-write compressor is not called
            assert len(calls) == n_calls and log and all(log) and timings["deflate_seconds"] > 0
        if name == "rh":                                        # --route device --deflate host: plain route calls, the host compresses
            assert log and not any(log) and "deflate_seconds" not in timings
        assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]


def test_malformed_input_leaves_no_output_file(tmp_path, capsys):
    from jasper_amd import triobin
    th.write_formats(tmp_path)
    (tmp_path / "bad.fq").write_bytes(ref.fastq_text(th.READS)[:-14])
    before = set(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        triobin.bin_files([str(tmp_path / "a.fq"), str(tmp_path / "bad.fq")], str(tmp_path / "out"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, write_gz=True)
    assert e.value.code == 1 and "record 5 is malformed" in capsys.readouterr().err
    assert set(os.listdir(tmp_path)) == before


def test_a_file_that_changes_between_the_passes_leaves_no_output_file(tmp_path, capsys):
    from jasper_amd import triobin
    path = tmp_path / "a.fq"
    path.write_bytes(ref.fastq_text(th.READS))
    calls = []

    def count(text, offs):
        if not calls:
            path.write_bytes(ref.fastq_text(th.READS[:3]))      # the second pass finds fewer records
        calls.append(1)
        return th.ref_counter()(text, offs)

    before = set(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        triobin.bin_files([str(path)], str(tmp_path / "out"), count, th.M_TOTAL, th.P_TOTAL, write_reads=True, write_gz=True)
    assert e.value.code == 1 and "changed between the two passes" in capsys.readouterr().err
    assert set(os.listdir(tmp_path)) == before


def test_without_the_flag_the_files_are_plain(tmp_path):
    from jasper_amd import triobin
    files = th.write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    timings = {}
    triobin.bin_files(paths, str(tmp_path / "p"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, write_reads=True, timings=timings)
    made = sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("p."))
    assert made == sorted(["p.readbins.tsv"] + ["p.%s.%s" % (b, fn[:-3] if fn.endswith(".gz") else fn) for b in ref.BINS for fn in files])
    assert not [fn for fn in made if fn.endswith(".gz")] and "deflate_raw" not in timings
    data = b"".join(open(tmp_path / ("p.%s.a.fq" % b), "rb").read() for b in ref.BINS)
    assert sorted(th.records_of(data)) == sorted(th.records_of(files["a.fq"]))


def test_every_bin_file_is_closed_when_closing_one_fails(tmp_path):
    """the end marker of the first file does not fit the disk: the two others are still ended and closed, and the error leaves"""
    from jasper_amd import triobin
    made = []
    files = triobin._BinFiles(str(tmp_path / "x"), "in.fq", made, write_gz=True)
    handles = [w.f for w in files.w]

    class Full:
        def __init__(self, f):
            self.f, self.closed = f, False

        def write(self, data):
            raise OSError(28, "No space left on device")

        def close(self):
            self.closed = True
            self.f.close()

    files.w[0].f = Full(handles[0])
    with pytest.raises(OSError, match="No space left"):
        files.close()
    assert files.w == [] and all(h.closed for h in handles)
    assert [os.path.getsize(fn + ".tmp") for fn in made] == [0, 28, 28]
    files.close()                                               # and closing again does nothing


def test_timing_line(capsys, monkeypatch):
    from jasper_amd import extensions, triobin
    lines = []
    monkeypatch.setattr(extensions, "device_line", lines.append)
    triobin.timing_lines({"deflate_raw": 100, "deflate_written": 40, "deflate_seconds": 0.5, "deflate_blocks": {"stored": 1, "literal_only": 2, "lz": 3}}, "host", "host", "device")
    assert lines == ["[triobin] deflate device: kernels device seconds 0.500000; 100 raw bytes, 40 compressed bytes; blocks stored 1, literal-only 2, LZ 3"]
    del lines[:]
    triobin.timing_lines({"deflate_raw": 100, "deflate_written": 40}, "host", "host", "host")
    assert lines == ["[triobin] deflate host: kernels device seconds NA; 100 raw bytes, 40 compressed bytes; blocks stored NA, literal-only NA, LZ NA"]
    del lines[:]
    triobin.timing_lines({}, "host", "host")                    # without --write-gz: no line
    assert lines == []


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("plan") / "deflate_plan_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "deflate_plan_check.cpp"), "-o", out])
    return out


def test_plan_header_under_the_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 16 and not r.stderr
