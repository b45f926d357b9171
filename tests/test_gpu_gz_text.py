"""GPU: a gzip text session (KmerTable.gz_text, jasper_gz_text_open / _bins / _copy / _stats) against the path that existed before it:
for every file the per-record arrays over all calls equal those of KmerTable.read_bins_text fed the decompressed bytes in the same
chunking -- the tail carried over, then `want` more -- and equal the restatements (tests/readtext_ref.py for the records,
tests/readbins_ref.py for the counters), so nothing is compared with the session's own output alone.

What can go wrong is where the inflater's slabs, the host-filled gaps, the calls and the carried tail meet: the files are written at
several levels, in several members, as fixed-Huffman and stored blocks (which the device leaves to the host), with slabs of 1 MB under a
file of more than 2 MB, and read with `want` from 1 byte to more than the file."""
import zlib

import numpy as np
import pytest

import readtext_ref as rt
from test_gpu_read_text import THRE, Trio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trio(hip):
    from jasper_amd import KmerTable
    t = Trio(KmerTable)
    yield t
    t.M.close()
    t.P.close()


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return co.compress(data) + co.flush()


def write(tmp_path, name, blob):
    p = tmp_path / name
    p.write_bytes(blob)
    return str(p)


def drive(t, path, data, want, fmt):
    """the session over the whole file next to read_bins_text over the same chunks -> (the session's stats, its calls); every call and
    the whole are compared here"""
    from jasper_amd import KmerTable
    got = {k: [] for k in ("lens", "mat", "pat", "starts", "head_end")}
    carry, pos, base, f, calls = b"", 0, 0, None, 0
    with t.M.gz_text(path) as g:
        while True:
            r = g.bins(t.P, want, f, THRE, THRE)
            calls += 1
            assert calls < 400000
            chunk = carry + data[pos:pos + want]
            pos = min(pos + want, len(data))
            assert g.n == len(chunk) and (not g.eof or pos == len(data))
            assert not r.no_format and not r.malformed
            if f is None and g.n:
                f = g.fmt
                assert f == fmt
            if calls % 7 == 1 and g.n:                  # the text itself, now and then: its two ends
                assert g.text(0, min(g.n, 100)).tobytes() == chunk[:100] and g.text(max(0, g.n - 100), min(g.n, 100)).tobytes() == chunk[-100:]
            want_r = KmerTable.read_bins_text(t.M, t.P, chunk, g.eof, fmt, THRE, THRE)      # (it writes the text slot: the session's tail is elsewhere)
            assert (r.used, r.n_records) == (want_r.used, want_r.n_records)
            for k, a, b in (("lens", r.lens, want_r.lens), ("mat", r.mat, want_r.mat), ("pat", r.pat, want_r.pat), ("starts", r.rec_start, want_r.rec_start),
                            ("head_end", r.head_end, want_r.head_end)):
                assert a.tolist() == b.tolist(), (k, calls)
                got[k].append((a[:-1] if k == "starts" else a) + (base if k in ("starts", "head_end") else 0))
            carry = chunk[r.used:]
            base += r.used
            if g.eof:
                break
        st = g.stats()
    assert pos == len(data) and not carry
    used, rec_start, head_end, lens, seq = rt.parse(data, True, fmt)
    cat = lambda k: np.concatenate(got[k]).tolist()     # noqa: E731
    assert cat("starts") == rec_start[:-1] and cat("head_end") == head_end and cat("lens") == lens
    m, p = t.counts(rt.reads_of(lens, seq))
    assert cat("mat") == m and cat("pat") == p and sum(m) + sum(p) > 0
    assert st["device_bytes"] + st["host_bytes"] == len(data)
    return st, calls


def fastq(trio, reps=10):
    return trio.cases["a"][1] * reps


def test_levels_and_members(trio, tmp_path):
    data = fastq(trio)
    assert 200000 < len(data) < 400000
    for level in (1, 6, 9):
        st, _ = drive(trio, write(tmp_path, "l%d.fq.gz" % level, gz(data, level)), data, 100000, "fastq")
        assert st["device_bytes"] == len(data) and st["members"] == 1
    cuts = [0, 1, len(data) // 3, len(data) // 2, len(data) - 7, len(data)]
    st, _ = drive(trio, write(tmp_path, "five.fq.gz", b"".join(gz(data[a:b]) for a, b in zip(cuts, cuts[1:]))), data, 100000, "fastq")
    assert st["members"] == 5


def test_blocks_the_device_leaves_to_the_host(trio, tmp_path, monkeypatch):
    """fixed-Huffman and stored blocks carry no header the start search finds: the first decoder runs until its arena is full (16 symbols
    per compressed byte of a chunk: 64 k with chunks of 4096 bytes, a quarter of this text) and zlib on the host fills the rest:
    host_bytes > 0, read_device's host-to-device branch"""
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_CHUNK", "4096")
    data = fastq(trio)
    for name, blob in (("fixed", gz(data, 6, zlib.Z_FIXED)), ("stored", gz(data, 0))):
        st, _ = drive(trio, write(tmp_path, name + ".fq.gz", blob), data, 70000, "fastq")
        assert st["host_bytes"] > 0, name


@pytest.fixture(scope="module")
def big(trio):
    """FASTQ of the trio's reads with random quality lines, so that more than 2 MB of compressed bytes come from 5.3 MB of text"""
    rng = np.random.default_rng(3)
    seqs = [s for _, s in trio.trio["r1"] if len(s) == 150][:80]
    qual = rng.integers(33, 127, (17000, 150), dtype=np.uint8)
    data = b"".join(b"@q%d\n" % i + seqs[i % 80] + b"\n+\n" + qual[i].tobytes() + b"\n" for i in range(17000))
    blob = gz(data)
    assert len(blob) > 2 << 20
    return data, blob


def test_slab_seams_inside_records(trio, big, tmp_path, monkeypatch):
    data, blob = big
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_CHUNK", "4096")
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_SLAB_MB", "1")
    st, _ = drive(trio, write(tmp_path, "big.fq.gz", blob), data, 1 << 20, "fastq")
    assert st["slabs"] >= 3


def test_small_wants(trio, tmp_path):
    """1000 bytes a call: every call carries a tail; 1 byte a call: progress still happens"""
    data = fastq(trio, 2)
    _, calls = drive(trio, write(tmp_path, "w1000.fq.gz", gz(data)), data, 1000, "fastq")
    assert calls >= len(data) // 1000
    tiny = trio.cases["a"][1][:trio.cases["a"][1].index(b"@", 600)]
    assert tiny.count(b"\n") % 4 == 0 and len(tiny) > 600
    _, calls = drive(trio, write(tmp_path, "w1.fq.gz", gz(tiny)), tiny, 1, "fastq")
    assert calls >= len(tiny)


def test_fasta_long_record_line_ends(trio, tmp_path):
    hap = trio.trio["hap_a"]
    long_seq = (hap * (100000 // len(hap) + 1))[:100000]
    long_fa = b">before\n" + hap[:150] + b"\n>long one\n" + b"".join(long_seq[i:i + 70] + b"\n" for i in range(0, 100000, 70)) + b">after\n" + hap[300:450] + b"\n"
    drive(trio, write(tmp_path, "long.fa.gz", gz(long_fa)), long_fa, 30000, "fasta")       # the record is longer than want: the tail grows
    for name in ("f_fasta", "f_fasta_crlf", "f_fasta_no_last_lf", "b_crlf", "b_no_last_lf", "b_last_cr_no_lf", "e_long_read"):
        fmt, text, _ = trio.cases[name]
        for want in (5000, 1 << 20):
            drive(trio, write(tmp_path, "%s_%d.gz" % (name, want), gz(text)), text, want, fmt)


def test_no_format_and_malformed(trio, tmp_path):
    from jasper_amd import KmerTable
    with trio.M.gz_text(write(tmp_path, "text.gz", gz(b"hello\n" + fastq(trio, 1)))) as g:
        r = g.bins(trio.P, 1000, None, THRE, THRE)
        assert r.no_format and not r.malformed and r.n_records == 0 and g.fmt is None and g.n == 1000 and r.mat is None
    # a wrong + line in the third chunk: the verdict and the record are the host-text path's for that chunk
    recs = rt.base_records(trio.trio) * 10
    lines = recs[560].split(b"\n")
    recs[560] = b"\n".join([lines[0], lines[1], b"-", lines[3], b""])
    data, want = b"".join(recs), 80000
    assert 2 * want < sum(map(len, recs[:560])) < 3 * want
    carry, pos = b"", 0
    with trio.M.gz_text(write(tmp_path, "bad.fq.gz", gz(data))) as g:
        for call in range(3):
            r = g.bins(trio.P, want, None if call == 0 else "fastq", THRE, THRE)
            chunk = carry + data[pos:pos + want]
            pos += want
            assert g.n == len(chunk) and g.text(0, g.n).tobytes() == chunk
            w = KmerTable.read_bins_text(trio.M, trio.P, chunk, g.eof, "fastq", THRE, THRE)
            assert (r.malformed, r.bad_record) == (w.malformed, w.bad_record) and r.malformed == (call == 2)
            carry = chunk[r.used:]
        with pytest.raises(rt.Bad) as e:
            rt.parse(chunk, False, "fastq")
        assert e.value.record == r.bad_record and e.value.what == rt.NO_PLUS


def records_until_error(t, path, want):
    """-> (lens, mat, pat of the records handed out, how the session ended: "error" = a call failed with a message that names the file,
    "verdict" = the parser called the text malformed or without a format, None = the file's end)"""
    from jasper_amd import _lib
    out, f = [], None
    with t.M.gz_text(path) as g:
        try:
            for _ in range(10000):
                r = g.bins(t.P, want, f, THRE, THRE)
                if r.malformed or r.no_format:
                    return out, "verdict"
                f = g.fmt
                out += list(zip(r.lens.tolist(), r.mat.tolist(), r.pat.tolist()))
                if g.eof:
                    return out, None
        except _lib.JasperHipError as e:
            assert path in str(e)                       # the message names the file
            with pytest.raises(_lib.JasperHipError):    # and the session stays failed
                g.bins(t.P, want, f, THRE, THRE)
            return out, "error"
    raise AssertionError("the session does not end")


def test_damaged_files_give_an_error_and_no_wrong_record(trio, big, tmp_path, monkeypatch):
    data, blob = big
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_SLAB_MB", "1")
    _, _, _, lens, seq = rt.parse(data, True, "fastq")
    m, p = trio.counts(rt.reads_of(lens, seq))
    truth = list(zip(lens, m, p))
    crc = bytearray(blob)
    crc[-8] ^= 1
    damaged = bytearray(blob)
    at = (1 << 20) + (1 << 19)                          # in the second slab
    damaged[at:at + 64] = b"\xff" * 64
    d = zlib.decompressobj(31)
    before = len(d.decompress(blob[:at]))               # text the bytes before the damage give
    for name, b, most in (("crc", bytes(crc), len(truth)), ("truncated", blob[:-(1 << 19)], len(truth)), ("damaged", bytes(damaged), before // 300)):
        got, ended = records_until_error(trio, write(tmp_path, name + ".fq.gz", b), 1 << 20)
        # a wrong CRC and a stream that stops are the inflater's to find: an error.  Bytes overwritten in the middle may decode to
        # text first, which the parser then refuses: either way no record of it is handed out
        assert ended == "error" if name != "damaged" else ended in ("error", "verdict"), (name, ended)
        assert got == truth[:len(got)] and len(got) <= most, name
    good, ended = records_until_error(trio, write(tmp_path, "good.fq.gz", blob), 1 << 20)
    assert ended is None and good == truth


def test_open_refuses_what_is_no_gzip_file(trio, tmp_path):
    from jasper_amd import _lib
    for name, blob in (("plain.fq", fastq(trio, 1)), ("short.gz", b"\x1f\x8b"), ("plain_named.gz", fastq(trio, 1))):
        with pytest.raises(_lib.JasperHipError, match="not for the device inflater"):
            trio.M.gz_text(write(tmp_path, name, blob))
    with pytest.raises(_lib.JasperHipError):
        trio.M.gz_text(str(tmp_path))                   # a directory
    st, _ = drive(trio, write(tmp_path, "after.fq.gz", gz(fastq(trio, 1))), fastq(trio, 1), 50000, "fastq")      # and the table is as good as before
    assert st["device_bytes"] > 0


def test_a_session_serves_bins_or_route_not_both(trio, tmp_path):
    """route has no tail to carry: a session that has parsed refuses to route, and one that has routed refuses to parse"""
    from jasper_amd import _lib
    data = fastq(trio, 1)
    bounds, bins = [0, 100, len(data)], [0, 2]
    with trio.M.gz_text(write(tmp_path, "a.fq.gz", gz(data))) as g:
        r = g.route(len(data), bounds, bins, b"@")
        assert r.routed and r.out[0].tobytes() == data[:100] and r.out[2].tobytes() == data[100:] and len(r.out[1]) == 0
        with pytest.raises(_lib.JasperHipError, match="not both"):
            g.bins(trio.P, 1000, None, THRE, THRE)
    with trio.M.gz_text(write(tmp_path, "b.fq.gz", gz(data))) as g:
        assert g.bins(trio.P, 1000, None, THRE, THRE).n_records > 0
        with pytest.raises(_lib.JasperHipError, match="not both"):
            g.route(len(data), bounds, bins, b"@")
