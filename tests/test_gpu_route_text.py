"""GPU: the routing kernels (KmerTable.route_text, jasper_route_text; a gz session's route, jasper_gz_text_route) against the numpy
restatement (tests/readroute_ref.py, itself checked on the CPU by tests/test_readroute_ref.py).  Nothing expected here comes from the
code under test.

What the kernels can get wrong is where segments, 16-byte thread spans and 4096-byte blocks meet, and where the segment scans change
blocks and passes: the texts hold empty segments, segments of 1 / 15 / 16 / 17 bytes, one 100 kb segment between short ones, texts
and segment counts at a block's edge, segment counts around one pass of the top scan, and every alignment of the text."""
import ctypes as C
import zlib

import numpy as np
import pytest

import readroute_ref as rr

pytestmark = pytest.mark.gpu


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
        assert r.out[b].tobytes() == outs[b], b
    assert r.mismatches == bad


@pytest.mark.parametrize("name", rr.CASE_NAMES)
def test_route_equals_the_restatement(table, cases, name):
    text, bounds, bins, check_from, planted, want = cases[name]
    assert want[1] == planted
    r = table.route_text(text, bounds, bins, rr.FIRST, check_from)
    check(r, want)
    assert r.seconds > 0


def test_every_alignment_of_the_text(table, cases):
    text, bounds, bins, check_from, _, want = cases["small_sizes"]
    room = np.zeros(len(text) + 64, dtype=np.uint8)
    base = (-room.ctypes.data) % 16                     # room[base] lies on a 16-byte boundary
    out = [np.empty(len(text), dtype=np.uint8) for _ in range(3)]
    for shift in range(16):
        view = room[base + shift:base + shift + len(text)]
        view[:] = np.frombuffer(text, dtype=np.uint8)
        assert view.ctypes.data % 16 == shift
        check(table.route_text(view, bounds, bins, rr.FIRST, check_from, out=out), want)


def test_refusals_are_host_checks(table):
    from jasper_amd import _lib
    text, bounds, bins = rr.build([10, 20, 30], [0, 1, 2], 1)
    for bad_bounds in ([1, 10, 30, 60], [0, 10, 30, 59], [0, 40, 30, 60], [0, -1, 30, 60]):
        with pytest.raises(_lib.JasperHipError, match="bounds"):
            table.route_text(text, bad_bounds, bins, rr.FIRST)
    with pytest.raises(_lib.JasperHipError, match="bin code"):
        table.route_text(text, bounds, [0, 3, 1], rr.FIRST)
    with pytest.raises(ValueError):
        table.route_text(text, bounds, [0, 1], rr.FIRST)
    L = _lib.lib()
    nb, bad = (C.c_int64 * 3)(), C.c_int64(0)
    zero = (C.c_int64 * 1)(0)
    for n in (1 << 31, 1 << 40):                        # a length, not a buffer: refused before anything is looked at
        assert L.jasper_route_text(table._h, None, n, 1, zero, None, 64, 0, None, None, None, nb, C.byref(bad), None) != 0
        assert "2^31" in L.jasper_last_error().decode()
    empty = table.route_text(b"", [0], [], rr.FIRST)
    assert [len(o) for o in empty.out] == [0, 0, 0] and empty.mismatches == 0
    check(table.route_text(text, bounds, bins, rr.FIRST), rr.route(text, bounds, bins))      # and the workspace is as good as before


def gz_file(tmp_path, name, data, level=6):
    path = tmp_path / name
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    path.write_bytes(co.compress(data) + co.flush())
    return str(path)


def test_session_route_in_blocks(table, cases, tmp_path):
    """a .gz file routed block by block: the blocks cut segments, so each block's bounds are the clipped ones"""
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
            r = g.route(end - at, b, bins[i0:i1], rr.FIRST, check_from)
            assert r.routed and r.got == end - at
            check(r, rr.route(text[at:end], b, bins[i0:i1], rr.FIRST, check_from))
            assert r.mismatches == 0
            for k in range(3):
                got[k] += r.out[k].tobytes()
        last = g.route(1, [0], [], rr.FIRST)
        assert last.got == 0 and last.routed
        st = g.stats()
    assert [bytes(x) for x in got] == rr.route(text, bounds, bins)[0]
    assert st["device_bytes"] + st["host_bytes"] == len(text) and st["device_bytes"] > 0


def test_session_route_of_a_file_that_is_not_the_bounds(table, cases, tmp_path):
    text, bounds, bins, check_from, _, want = cases["long_record"]
    with table.gz_text(gz_file(tmp_path, "short.gz", text[:-5])) as g:
        r = g.route(len(text), bounds, bins, rr.FIRST, check_from)
        assert not r.routed and r.got == len(text) - 5 and r.out is None
    with table.gz_text(gz_file(tmp_path, "long.gz", text + b"@more")) as g:
        check(g.route(len(text), bounds, bins, rr.FIRST, check_from), want)
        r = g.route(1, [0], [], rr.FIRST)
        assert r.got == 1 and not r.routed              # bytes are left over
    with table.gz_text(gz_file(tmp_path, "same.gz", text)) as g:
        check(g.route(len(text), bounds, bins, rr.FIRST, check_from), want)
