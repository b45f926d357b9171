"""CPU: the host side of `python -m jasper_amd.triobin --gz device / --route device` -- the flags, the arithmetic that cuts a block of
the second pass into segments, the plan header of the routing path under a sanitizer, and the tool's two passes over a gzip text session.
The GPU's parts are replaced by the restatements (tests/readtext_ref.py, tests/readbins_ref.py, tests/readroute_ref.py), as
test_triobin_reader_host.py replaces the parser; tests/test_gpu_cli_triobin_gz.py runs the real ones."""
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import readbins_ref as ref
import readroute_ref as rr
import test_triobin_host as th
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
        (["--gz", "x"], "--gz takes host or device; x was given"),
        (["--reader", "device", "--gz", "gpu"], "--gz takes host or device; gpu was given"),
        (["--route", "both", "--reader", "device", "--write-reads"], "--route takes host or device; both was given"),
        (["--gz", "device"], "--gz device needs --reader device"),
        (["--gz", "device", "--reader", "host"], "--gz device needs --reader device"),
        (["--route", "device"], "--route device needs --reader device --write-reads"),
        (["--route", "device", "--reader", "device"], "--route device needs --reader device --write-reads"),
        (["--route", "device", "--write-reads"], "--route device needs --reader device --write-reads"),
        (["--route", "device", "--write-reads", "--reader", "host", "--gz", "host"], "--route device needs --reader device --write-reads"),
    ]
    before = sorted(os.listdir(tmp_path))
    for extra, message in cases:
        with pytest.raises(SystemExit) as e:
            triobin.run(base + extra)
        assert e.value.code == 1, extra
        assert message in capsys.readouterr().err, extra
        assert sorted(os.listdir(tmp_path)) == before, extra
    ok = triobin.parse_args(base + ["--reader", "device", "--write-reads", "--gz", "device", "--route", "device"])
    assert triobin.check_gz_route(ok, "device") == ("device", "device")
    assert triobin.check_gz_route(triobin.parse_args(base), "host") == ("host", "host")
    assert triobin.check_gz_route(triobin.parse_args(base + ["--gz", "host", "--route", "host"]), "host") == ("host", "host")
    assert "--gz host|device" in triobin.USAGE and "--route host|device" in triobin.USAGE


def brute_segments(starts, length, at, end):
    """which record every byte of [at, end) lies in, one byte at a time -> (i0, i1, bounds, check_from)"""
    owner = []
    for pos in range(at, end):
        owner.append(max(i for i, s in enumerate(starts) if s <= pos))
    i0, i1 = owner[0], owner[-1] + 1
    bounds = [0] + [k for k in range(1, len(owner)) if owner[k] != owner[k - 1]] + [end - at]
    return i0, i1, bounds, 0 if at in starts else 1


def test_block_segments_equal_a_byte_by_byte_restatement():
    from jasper_amd import triobin
    sizes = [30, 1, 45, 200, 7, 7, 64, 3, 120, 11]
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    length = int(sum(sizes))
    shapes = set()
    for block in (1, 5, 7, 29, 30, 31, 64, 100, 199, 201, length - 1, length, length + 50):
        for at in range(0, length, block):
            end = min(at + block, length)
            i0, i1, bounds, check_from = triobin.block_segments(starts, at, end)
            assert (i0, i1, bounds.tolist(), check_from) == brute_segments(starts.tolist(), length, at, end), (block, at)
            assert bounds.dtype == np.int64 and len(bounds) == i1 - i0 + 1
            clipped_front, clipped_back = check_from == 1, end < length and end not in starts.tolist()
            shapes.add((clipped_front, clipped_back, i1 - i0 == 1))
    # blocks that clip a record at both ends, with and without whole records between, and a block inside one record
    assert {(True, True, True), (True, True, False), (False, False, False), (False, True, True), (True, False, True)} <= shapes


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("plan") / "readroute_plan_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "readroute_plan_check.cpp"), "-o", out])
    return out


def test_plan_header_under_the_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 15 and not r.stderr


# ---- the tool's two passes over a session that is the restatements -------------------------------------------------------------------
class FakeSession:
    """what table.GzText gives the tool, from the decompressed bytes: bins(want, fmt) carries the tail; route(...) pulls the next bytes"""

    def __init__(self, path, log):
        with gzip.open(path, "rb") as f:
            self.data = f.read()
        self.path, self.log, self.pos, self.tail, self.cur = path, log, 0, b"", b""
        self.n, self.eof, self.fmt, self.inflate_seconds, self.closed = 0, False, None, 0.0, False

    def bins(self, want, fmt):
        assert not self.closed and fmt == self.fmt
        new = self.data[self.pos:self.pos + want]
        self.pos += len(new)
        self.cur = self.tail + new
        self.n, self.eof = len(self.cur), len(new) < want
        r = types.SimpleNamespace(malformed=False, no_format=False, bad_record=-1, seconds=0.0, index_seconds=0.0, used=0, n_records=0)
        if self.fmt is None and self.n:
            self.fmt = {b"@": "fastq", b">": "fasta"}.get(self.cur[:1])
            if self.fmt is None:
                r.no_format = True
                return r
        if not self.n:
            return r
        r2 = fake_count_text()(np.frombuffer(self.cur, dtype=np.uint8), self.eof, self.fmt)
        self.tail = self.cur if r2.malformed else self.cur[r2.used:]
        r2.no_format = False
        return r2

    def text(self, start, length):
        assert 0 <= start and start + length <= self.n
        self.log.append(("text", self.path, start, length))
        return np.frombuffer(self.cur[start:start + length], dtype=np.uint8)

    def route(self, want, bounds, bins, first, check_from, out):
        assert not self.closed
        new = self.data[self.pos:self.pos + want]
        self.pos += len(new)
        self.log.append(("route", self.path, want))
        if len(new) != bounds[-1]:
            return types.SimpleNamespace(out=None, mismatches=0, seconds=0.0, got=len(new), routed=False)
        outs, bad = rr.route(new, bounds, bins, first[0] if len(first) else 0, check_from)
        return types.SimpleNamespace(out=[np.frombuffer(o, dtype=np.uint8) for o in outs], mismatches=bad, seconds=0.0, got=len(new), routed=True)

    def stats(self):
        return {"device_bytes": self.pos, "host_bytes": 0}

    def close(self):
        self.closed = True


def fake_route_text(log):
    def route_text(buf, bounds, bins, first, check_from, out):
        log.append(("route_text", len(buf)))
        outs, bad = rr.route(buf.tobytes(), bounds, bins, first[0], check_from)
        return types.SimpleNamespace(out=[np.frombuffer(o, dtype=np.uint8) for o in outs], mismatches=bad, seconds=0.0)
    return route_text


def test_both_passes_over_a_session_write_what_the_host_reader_writes(tmp_path, monkeypatch):
    from jasper_amd import triobin
    files = th.write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    host = str(tmp_path / "host")
    triobin.bin_files(paths, host, th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True)
    outs = sorted(fn[len("host"):] for fn in os.listdir(tmp_path) if fn.startswith("host."))
    for chunk, per_read, route in ((None, True, True), (64, True, True), (7, False, True), (1, True, True), (9, True, False)):
        if chunk is None:
            monkeypatch.delenv("JASPER_TRIOBIN_CHUNK", raising=False)
        else:
            monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", str(chunk))
        monkeypatch.setattr(triobin, "CHUNK", 16 << 20 if chunk is None else 5 * chunk + 3)      # (the second pass's blocks)
        log, sessions, timings = [], [], {}

        def gz_open(path):
            sessions.append(FakeSession(path, log))
            return sessions[-1]

        prefix = str(tmp_path / ("dev%s" % chunk))
        triobin.bin_files(paths, prefix, never, th.M_TOTAL, th.P_TOTAL, per_read=per_read, write_reads=True, reader="device", count_text=fake_count_text(), gz_open=gz_open,
                          route_text=fake_route_text(log) if route else None, timings=timings)
        for tail in outs:
            if per_read or not tail.endswith(".reads.tsv"):
                assert open(prefix + tail, "rb").read() == open(host + tail, "rb").read(), (chunk, tail)
        assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]
        gz = [p for p in paths if p.endswith(".gz")]
        assert [s.path for s in sessions] == gz * (2 if route else 1) and all(s.closed for s in sessions)      # a session a pass, none for a plain file
        assert [p for p, _ in timings["gz_stats"]] == gz
        texts = [e for e in log if e[0] == "text"]
        assert bool(texts) == per_read                  # the text comes back for the names alone
        assert ("route_text" in {e[0] for e in log}) == route and ("route" in {e[0] for e in log}) == route
        for fn in os.listdir(tmp_path):
            if fn.startswith("dev%s." % chunk):
                os.remove(tmp_path / fn)


def test_a_session_that_fails_ends_the_run_and_names_the_file(tmp_path, capsys):
    from jasper_amd import triobin
    th.write_formats(tmp_path)
    path = str(tmp_path / "f.fq.gz")

    class Failing(FakeSession):
        def bins(self, want, fmt):
            if self.pos:
                raise RuntimeError("crc or length error in " + self.path)
            return FakeSession.bins(self, want, fmt)

    os.environ["JASPER_TRIOBIN_CHUNK"] = "40"
    try:
        before = set(os.listdir(tmp_path))
        with pytest.raises(SystemExit) as e:
            triobin.bin_files([path], str(tmp_path / "out"), never, th.M_TOTAL, th.P_TOTAL, write_reads=True, reader="device", count_text=fake_count_text(),
                              gz_open=lambda p: Failing(p, []))
        err = capsys.readouterr().err
        assert e.value.code == 1 and "f.fq.gz: the gzip stream cannot be inflated" in err and "crc or length error" in err
        assert set(os.listdir(tmp_path)) == before
    finally:
        del os.environ["JASPER_TRIOBIN_CHUNK"]


def test_second_pass_over_a_session_notices_a_changed_file(tmp_path, capsys):
    from jasper_amd import triobin
    data = ref.fastq_text(th.READS)
    path = tmp_path / "a.fq.gz"
    shifted = data.replace(b"@", b"@x", 1)[:len(data)]
    for changed in (data + ref.fastq_text(th.READS[:1]), data[:-9], shifted):
        path.write_bytes(gzip.compress(data))
        opened = []

        def gz_open(p):
            if opened:                                  # the second pass opens another file under the name
                path.write_bytes(gzip.compress(changed))
            opened.append(p)
            return FakeSession(p, [])

        before = set(os.listdir(tmp_path))
        with pytest.raises(SystemExit) as e:
            triobin.bin_files([str(path)], str(tmp_path / "out"), never, th.M_TOTAL, th.P_TOTAL, write_reads=True, reader="device", count_text=fake_count_text(),
                              gz_open=gz_open, route_text=fake_route_text([]))
        assert e.value.code == 1 and "changed between the two passes" in capsys.readouterr().err and len(opened) == 2
        assert set(os.listdir(tmp_path)) == before
