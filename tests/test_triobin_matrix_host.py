"""CPU: `triobin.bin_files` with the device reader over every combination of where a block's text comes from and what leaves the router
-- a gzip text session or the host's buffer, route_text or the host's masks, plain files or BGZF from zlib or from a compressor handed in
-- at chunk sizes that cut every record.  Each source and each writer has a test file of its own (test_triobin_reader_host.py,
test_triobin_gz_host.py, test_triobin_write_gz_host.py); this one holds the one chunk loop and the one block loop against all of them at
once.  The GPU's parts are those files' stand-ins."""
import gzip
import itertools
import os

import numpy as np
import pytest

import test_triobin_host as th
from test_triobin_reader_host import fake_count_text, never
from test_triobin_write_gz_host import FakeSessionGz, fake_route_text_gz

WRITERS = ("plain", "zlib", "deflate")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """FASTQ, FASTA, CRLF, .gz and files whose last line has no LF, and what the host reader writes for them"""
    from jasper_amd import triobin
    d = tmp_path_factory.mktemp("matrix")
    files = th.write_formats(d)
    paths = [str(d / fn) for fn in files]
    triobin.bin_files(paths, str(d / "host"), th.ref_counter(), th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True)
    want = {fn[len("host"):]: open(d / fn, "rb").read() for fn in os.listdir(d) if fn.startswith("host.")}
    assert len(want) == 2 + 3 * len(paths)
    return d, paths, want


@pytest.mark.parametrize("chunk", [1, 7, 64])           # 1: a tail longer than a block; 7: blocks clipped at both ends
def test_every_source_router_and_writer_writes_what_the_host_reader_writes(host_run, monkeypatch, chunk):
    from jasper_amd import bgzf, triobin
    d, paths, want = host_run
    monkeypatch.setenv("JASPER_TRIOBIN_CHUNK", str(chunk))
    monkeypatch.setattr(triobin, "CHUNK", 5 * chunk + 3)
    gz_paths = [p for p in paths if p.endswith(".gz")]
    for n, (with_gz, with_route, writer) in enumerate(itertools.product((False, True), (False, True), WRITERS)):
        sessions, routed, deflated = [], [], []

        def gz_open(path):
            sessions.append(FakeSessionGz(path, []))
            return sessions[-1]

        def deflate(arr):
            deflated.append(len(arr))
            return np.frombuffer(bgzf.compress(arr), dtype=np.uint8), {"stored": 0, "literal_only": 0, "lz": 1}, 0.0

        prefix, case = str(d / ("m%d_%d" % (chunk, n))), (chunk, with_gz, with_route, writer)
        triobin.bin_files(paths, prefix, never, th.M_TOTAL, th.P_TOTAL, per_read=True, write_reads=True, reader="device", count_text=fake_count_text(),
                          gz_open=gz_open if with_gz else None, route_text=fake_route_text_gz(routed) if with_route else None, write_gz=writer != "plain",
                          deflate=deflate if writer == "deflate" else None)
        made = sorted(fn for fn in os.listdir(d) if fn.startswith(os.path.basename(prefix) + "."))
        assert len(made) == len(want), case
        for tail, data in want.items():
            if tail.endswith(".tsv") or writer == "plain":
                assert open(prefix + tail, "rb").read() == data, (case, tail)
            else:
                assert not os.path.exists(prefix + tail) and gzip.decompress(open(prefix + tail + ".gz", "rb").read()) == data, (case, tail)
        assert not [fn for fn in os.listdir(d) if fn.endswith(".tmp")], case
        # a session a pass and .gz file, the second pass's only beside route_text; every one of them closed
        assert [s.path for s in sessions] == gz_paths * ((2 if with_route else 1) if with_gz else 0) and all(s.closed for s in sessions), case
        assert bool(routed) == with_route and all(gz == (writer == "deflate") for gz in routed), case       # (the route calls compress only with a compressor)
        assert bool(deflated) == (writer == "deflate" and not with_route), case                             # ... and then no write does
        for fn in made:
            os.remove(d / fn)
