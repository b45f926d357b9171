"""GPU: the routing calls that compress their three outputs on the GPU (KmerTable.route_text(gz=True), jasper_route_text_gz; a gz
session's route(gz=True), jasper_gz_text_route_gz) on the shapes of tests/test_gpu_route_text.py.  Each bin's members go through the
strict walker (tests/bgzf_ref.py) and its text must be the numpy restatement's bytes (tests/readroute_ref.py); raw_bytes, mismatches and
got must be what the plain calls report."""
import numpy as np
import pytest

import bgzf_ref
import readroute_ref as rr
from test_gpu_route_text import gz_file

pytestmark = pytest.mark.gpu
BLOCK = 65280


@pytest.fixture(scope="module")
def table(hip):
    from jasper_amd import KmerTable
    t = KmerTable(21, min_slots=1 << 12)
    yield t
    t.close()


@pytest.fixture(scope="module")
def cases():
    c = rr.cases()
    return {name: v + (rr.route(v[0], v[1], v[2], rr.FIRST, v[3]),) for name, v in c.items()}


def check(r, want):
    outs, bad = want
    for b in range(3):
        assert bgzf_ref.members(r.out[b].tobytes()) == outs[b], b
        assert len(bgzf_ref.split(r.out[b].tobytes())) == -(-len(outs[b]) // BLOCK)      # a bin without a byte: no member
    assert r.raw_bytes == [len(o) for o in outs] and r.mismatches == bad
    assert r.deflate["blocks"] == sum(-(-len(o) // BLOCK) for o in outs)


@pytest.mark.parametrize("name", rr.CASE_NAMES)
def test_route_gz_equals_the_restatement(table, cases, name):
    text, bounds, bins, check_from, planted, want = cases[name]
    r = table.route_text(text, bounds, bins, rr.FIRST, check_from, gz=True)
    check(r, want)
    plain = table.route_text(text, bounds, bins, rr.FIRST, check_from)
    assert [len(o) for o in plain.out] == r.raw_bytes and plain.mismatches == r.mismatches == planted
    assert r.seconds > 0 and (r.deflate_seconds > 0) == (len(text) > 0)


def test_a_segment_across_the_member_seam_and_empty_bins(table):
    """one segment that begins before byte 65280 of its bin and ends behind it, bins 1 and 2 empty; then empty segments around it"""
    rng = np.random.default_rng(4)
    for sizes, bins in (([65000, 1000], [0, 0]), ([0, 65279, 0, 2, 0], [2, 2, 1, 2, 0]), ([BLOCK, BLOCK, 1], [1, 1, 1])):
        text = b"".join(b"@" + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, s - 1)].tobytes() if s else b"" for s in sizes)
        bounds = np.concatenate(([0], np.cumsum(sizes)))
        check(table.route_text(text, bounds, bins, rr.FIRST, gz=True), rr.route(text, bounds, np.array(bins, dtype=np.uint8)))
    empty = table.route_text(b"", [0], [], rr.FIRST, gz=True)
    assert [len(o) for o in empty.out] == [0, 0, 0] and empty.raw_bytes == [0, 0, 0] and empty.mismatches == 0 and empty.deflate["blocks"] == 0


def test_session_route_gz_in_blocks(table, cases, tmp_path):
    """a .gz file routed and compressed block by block; the concatenated members of each bin are one valid series"""
    text, bounds, bins, _, _, _ = cases["random"]
    path = gz_file(tmp_path, "r.gz", text)
    block = 150001
    got = [bytearray(), bytearray(), bytearray()]
    with table.gz_text(path) as g:
        for at in range(0, len(text), block):
            end = min(at + block, len(text))
            i0 = int(np.searchsorted(bounds, at, side="right")) - 1
            i1 = int(np.searchsorted(bounds, end, side="left"))
            b = np.concatenate(([0], bounds[i0 + 1:i1] - at, [end - at]))
            check_from = 0 if bounds[i0] == at else 1
            r = g.route(end - at, b, bins[i0:i1], rr.FIRST, check_from, gz=True)
            assert r.routed and r.got == end - at and r.mismatches == 0
            check(r, rr.route(text[at:end], b, bins[i0:i1], rr.FIRST, check_from))
            for k in range(3):
                got[k] += r.out[k].tobytes()
        last = g.route(1, [0], [], rr.FIRST, gz=True)
        assert last.got == 0 and last.routed and last.raw_bytes == [0, 0, 0]
    assert [bgzf_ref.members(bytes(x)) for x in got] == rr.route(text, bounds, bins)[0]
    with table.gz_text(gz_file(tmp_path, "short.gz", text[:-5])) as g:      # a file that is not the bounds: nothing is routed
        r = g.route(len(text), bounds, bins, rr.FIRST, gz=True)
        assert not r.routed and r.got == len(text) - 5 and r.out is None and r.raw_bytes == [0, 0, 0]
