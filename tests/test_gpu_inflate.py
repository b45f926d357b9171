"""GPU: one gzip stream inflated on the device (jasper_amd/csrc/inflate_gpu.hip through jasper_inflate_file_device, and inside
count_files / the read feed / the drop-in driver) against Python's gzip and the host readers.  Small decoder chunks
(JASPER_INGEST_GZ_DEVICE_CHUNK) give files of a few MB hundreds of decoders; the counters of jasper_last_inflate say which
engine produced the text."""
import ctypes as C
import gzip
import json
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHUNK = 16 << 10
KEYS = ("decoders", "accepted", "device_bytes", "host_bytes", "slabs", "members")


def fastq_text(seed, nreads, rl=150):
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3_000_000)]
    q = np.frombuffer(b"FFFFFFFF:F,F#", dtype=np.uint8)
    out = []
    for i in range(nreads):
        s = int(rng.integers(0, len(g) - rl))
        out.append(b"@SIM:1:FC:%d:%d 1:N:0:ACGT\n" % (i // 1000, i % 1000) + g[s:s + rl].tobytes() + b"\n+\n" + q[rng.integers(0, len(q), rl)].tobytes() + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def FQ():
    return fastq_text(1, 44_000)          # ~15 MB of text, 4-5 MB at levels 9-1: 120-160 deflate blocks


def dev_inflate(L, path, out=None, chunk=CHUNK):
    n = C.c_uint64(0)
    st = (C.c_uint64 * 6)()
    rc = L.jasper_inflate_file_device(0, str(path).encode(), chunk, str(out).encode() if out else None, C.byref(n), st)
    return rc, n.value, dict(zip(KEYS, (int(v) for v in st)))


def host_inflate(L, path, out=None):
    n = C.c_uint64(0)
    par = C.c_int(0)
    rc = L.jasper_inflate_file(str(path).encode(), 4, 1 << 16, str(out).encode() if out else None, C.byref(n), C.byref(par))
    return rc, n.value, par.value


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return co.compress(data) + co.flush()


def check_same(L, tmp_path, blob, text, device_only=True):
    p, out = tmp_path / "in.gz", tmp_path / "out"
    p.write_bytes(blob)
    rc, n, st = dev_inflate(L, p, out)
    assert rc == 0, st
    assert n == len(text) and out.read_bytes() == text
    assert st["device_bytes"] + st["host_bytes"] == len(text)
    if device_only:
        assert st["accepted"] >= 100 and st["host_bytes"] == 0, st
    return st


@pytest.mark.parametrize("level", [1, 6, 9])
def test_levels(hip, tmp_path, FQ, level):
    st = check_same(hip, tmp_path, gzip.compress(FQ, level, mtime=0), FQ)
    assert st["members"] == 1 and st["accepted"] <= st["decoders"]


@pytest.mark.parametrize("strategy", [zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE])
def test_strategies(hip, tmp_path, FQ, strategy):
    check_same(hip, tmp_path, gz(FQ, 6, strategy), FQ)


def test_blocks_without_a_findable_start(hip, tmp_path, FQ):
    """fixed-Huffman (Z_FIXED) and stored (level 0) blocks carry no header the start search can recognise: the first chunk is decoded
    on the device until its arena is full, zlib on the host fills the gap from that block start -- same bytes, and the counters say so"""
    for blob in (gz(FQ[:3_000_000], 6, zlib.Z_FIXED), gzip.compress(FQ[:3_000_000], 0, mtime=0)):
        st = check_same(hip, tmp_path, blob, FQ[:3_000_000], device_only=False)
        assert st["host_bytes"] > 0
    # within one chunk's arena those blocks are decoded on the device
    for blob in (gz(FQ[:60_000], 6, zlib.Z_FIXED), gzip.compress(FQ[:60_000], 0, mtime=0)):
        st = check_same(hip, tmp_path, blob, FQ[:60_000], device_only=False)
        assert st["host_bytes"] == 0 and st["device_bytes"] == 60_000


def test_members_and_headers(hip, tmp_path, FQ):
    a, b, c = FQ[:5_000_000], FQ[5_000_000:10_000_000], FQ[10_000_000:]
    blob = gzip.compress(a, 6, mtime=0) + gzip.compress(b, 1, mtime=0) + gzip.compress(b"", 6, mtime=0) + gzip.compress(b"", 9, mtime=0) + gzip.compress(c, 9, mtime=0)
    st = check_same(hip, tmp_path, blob, FQ)
    assert st["members"] == 5
    # bgzf-like: thousands of members of 4 KB of text
    parts = [FQ[i:i + 4096] for i in range(0, len(FQ), 4096)]
    st = check_same(hip, tmp_path, b"".join(gzip.compress(x, 6, mtime=0) for x in parts), FQ)
    assert st["members"] == len(parts)
    # member headers with FEXTRA, FNAME, FCOMMENT and FHCRC
    def member(data, flg):
        hdr = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03"
        if flg & 4:
            hdr += b"\x06\x00AB\x02\x00xy"
        if flg & 8:
            hdr += b"reads.fq\0"
        if flg & 16:
            hdr += b"a comment\0"
        if flg & 2:
            hdr += (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little")
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        return hdr + co.compress(data) + co.flush() + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")
    st = check_same(hip, tmp_path, member(a, 4 | 8 | 16 | 2) + member(b, 8) + member(c, 16 | 2), FQ)
    assert st["members"] == 3


def test_binary_data_and_trailing_bytes(hip, tmp_path, FQ):
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, 700_000, dtype=np.uint8).tobytes()
    mixed = FQ[:2_000_000] + noise + bytes(range(256)) * 2000 + FQ[2_000_000:4_000_000]
    check_same(hip, tmp_path, gzip.compress(mixed, 6, mtime=0), mixed, device_only=False)
    # after the last member: zero padding is skipped, anything else fails -- whatever jasper_inflate_file's many-thread reader does
    z = gzip.compress(FQ[:3_000_000], 6, mtime=0)
    p = tmp_path / "t.gz"
    for tail in (b"\0" * 100, b"\0\0junk", b"x", b"\x1f\x8b"):
        p.write_bytes(z + tail)
        rc_h, n_h, par = host_inflate(hip, p)
        rc_d, n_d, st = dev_inflate(hip, p)
        assert par == 1 and (rc_d == 0) == (rc_h == 0), tail
        if rc_d == 0:
            assert n_d == 3_000_000


def test_overflow_goes_to_the_host(hip, tmp_path):
    """10^8 'A's: every block far larger than a decoder's arena -- the host fills in from the last block start the device reached"""
    text = b"A" * 100_000_000
    p, out = tmp_path / "a.gz", tmp_path / "out"
    p.write_bytes(gzip.compress(text, 6, mtime=0))
    rc, n, st = dev_inflate(hip, p, out)
    assert rc == 0 and n == len(text) and st["host_bytes"] > 0
    assert out.read_bytes() == text


def test_false_starts_are_never_accepted(hip, tmp_path, FQ, monkeypatch):
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_FALSE_STARTS", "1")
    st = check_same(hip, tmp_path, gzip.compress(FQ, 6, mtime=0), FQ)
    assert st["accepted"] < st["decoders"] and st["decoders"] >= 2 * st["accepted"] - 2


def test_damaged_files_fail(hip, tmp_path, FQ):
    """truncated, a flipped bit, a wrong CRC, a wrong length: an error, never other text -- and the same verdict as the host reader"""
    z = gzip.compress(FQ[:4_000_000], 6, mtime=0)
    p = tmp_path / "d.gz"
    cases = [z[:cut] for cut in (len(z) // 3, len(z) // 2, len(z) - 4, len(z) - 9, len(z) - 1000)]
    crc_bad = bytearray(z)
    crc_bad[-6] ^= 0x10
    len_bad = bytearray(z)
    len_bad[-2] ^= 0x01
    cases += [bytes(crc_bad), bytes(len_bad)]
    rng = np.random.default_rng(8)
    for _ in range(10):
        f = bytearray(z)
        pos = int(rng.integers(len(z) // 10, len(z) - 100))
        f[pos] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(f))
    for i, blob in enumerate(cases):
        p.write_bytes(blob)
        rc_d, _, st = dev_inflate(hip, p)
        rc_h, _, _ = host_inflate(hip, p)
        assert rc_d != 0 and rc_h != 0, (i, st)


def fq_records(seed, n):
    from jasper_amd import synth
    rng = np.random.default_rng(seed)
    genome = synth.make_genome(rng, 200_000, repeat_frac=0)
    stream = synth.make_reads_stream(rng, genome, 40, 150, 0.004).tobytes().decode()
    reads = [r for r in stream.split("N") if r][:n]
    q = np.frombuffer(b"FFFFFFFF:F,F#", dtype=np.uint8)
    return b"".join(b"@r%d_%d\n%s\n+\n%s\n" % (seed, i, r.encode(), q[rng.integers(0, len(q), len(r))].tobytes()) for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def three_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gz3")
    t1, t2, t3 = fq_records(11, 6000), fq_records(12, 30000), fq_records(13, 7000)     # (b.fq.gz: more than 2 MB compressed, for 1 MB slabs)
    (d / "a.fq").write_bytes(t1)
    (d / "b.fq.gz").write_bytes(gzip.compress(t2, 6, mtime=0))
    (d / "c.fq.gz").write_bytes(gzip.compress(t3, 1, mtime=0))
    return [str(d / "a.fq"), str(d / "b.fq.gz"), str(d / "c.fq.gz")], t1 + t2 + t3, len(t2) + len(t3)


def test_count_files_device_host_oracle(hip, three_files, monkeypatch):
    from jasper_amd import KmerTable
    from oracle import oracle as O
    paths, text, gz_len = three_files
    k = 25
    db = O.OracleDB(k)
    db.count_text(text.decode())
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_CHUNK", str(CHUNK))
    res = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("JASPER_INGEST_GZ", mode)
        t = KmerTable(k, min_slots=1 << 20)
        t.count_files(paths)
        res[mode] = (t.histogram(), t.info()["distinct"], t.last_inflate())
        t.close()
    assert res["device"][0] == db.histo() and res["device"][1] == db.distinct()
    assert res["host"][:2] == res["device"][:2]
    assert res["device"][2]["device_bytes"] == gz_len and res["device"][2]["host_bytes"] == 0 and res["device"][2]["accepted"] > 2
    assert res["host"][2]["device_bytes"] == 0 and res["host"][2]["host_bytes"] == gz_len
    # the same through the read feed: batches of bases in HBM, counted by a second table
    monkeypatch.setenv("JASPER_INGEST_GZ", "device")
    src = KmerTable(k, min_slots=1 << 16)
    dst = KmerTable(k, min_slots=1 << 20)
    src.feed_start([(p, 0, -1) for p in paths])
    while True:
        ptr, n = src.feed_next()
        if n == 0:
            break
        dst.count_bases_device(ptr, n)
        src.feed_release()
    st = src.last_inflate()
    assert dst.histogram() == db.histo() and st["device_bytes"] == gz_len and st["host_bytes"] == 0
    src.close()
    dst.close()


def test_auto_selection(hip, three_files, monkeypatch):
    from jasper_amd import KmerTable
    paths, text, gz_len = three_files
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_CHUNK", str(CHUNK))
    monkeypatch.delenv("JASPER_INGEST_GZ", raising=False)
    t = KmerTable(25, min_slots=1 << 20)
    t.count_files(paths)                                   # default threshold: these files are far below it
    assert t.last_inflate()["device_bytes"] == 0
    h0 = t.histogram()
    t.clear()
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_MIN_MB", "0")
    t.count_files(paths)
    st = t.last_inflate()
    assert st["device_bytes"] == gz_len and st["host_bytes"] == 0 and t.histogram() == h0
    t.clear()
    monkeypatch.setenv("JASPER_INGEST_GZ", "host")
    t.count_files(paths)
    assert t.last_inflate()["device_bytes"] == 0 and t.histogram() == h0
    t.close()


def test_cli_gzip_reads_on_the_device(hip, tmp_path):
    """the drop-in driver on the golden run's own .fq.gz files, inflated on the device: the golden outputs"""
    E2E = os.path.join(HERE, "golden", "e2e")
    meta = json.load(open(os.path.join(E2E, "meta.json")))
    K = meta["k"]
    for fn in ("r1.fq.gz", "r2.fq.gz", "asm.fa"):
        shutil.copy(os.path.join(E2E, fn), tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, JASPER_INGEST_GZ="device", JASPER_INGEST_GZ_DEVICE_CHUNK=str(CHUNK))
    p = subprocess.run([sys.executable, "-m", "jasper_amd.cli", "-r", "r1.fq.gz r2.fq.gz", "-a", "asm.fa", "-k", str(K),
                        "-t", str(meta["threads"]), "-p", str(meta["passes"])],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert open(tmp_path / "threshold.txt").read() == open(os.path.join(E2E, "threshold.txt")).read()
    assert open(tmp_path / ("jfhisto%d.csv" % K)).read() == open(os.path.join(E2E, "jfhisto%d.csv" % K)).read()
    from test_gpu_cli_e2e import fasta_records
    assert fasta_records(tmp_path / "asm.fa.polished.fasta") == fasta_records(os.path.join(E2E, "asm.fa.polished.fasta"))
    assert open(tmp_path / "asm.fa.fixes.csv", newline="").read() == open(os.path.join(E2E, "asm.fa.fixes.csv"), newline="").read()


# ---- slab seams: with JASPER_INGEST_GZ_DEVICE_SLAB_MB=1 the files above are 3-5 slabs, as every real read file is many -----------------
# (what next_slab carries from one slab to the next: the position inside a 4096-byte page, the decoder that ends past the slab's nominal
# end, the window kept on the device or uploaded from the host after a gap, the member's CRC, length and valid window so far)
@pytest.fixture
def slab_1mb(monkeypatch):
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_SLAB_MB", "1")


@pytest.mark.parametrize("level", [1, 6, 9])
def test_slabs_levels(hip, tmp_path, FQ, slab_1mb, level):
    blob = gzip.compress(FQ, level, mtime=0)
    st = check_same(hip, tmp_path, blob, FQ)
    assert st["host_bytes"] == 0 and st["members"] == 1
    assert st["slabs"] >= max(3, len(blob) >> 20), st


def test_slabs_members(hip, tmp_path, FQ, slab_1mb):
    a, b, c = FQ[:5_000_000], FQ[5_000_000:10_000_000], FQ[10_000_000:]
    blob = gzip.compress(a, 6, mtime=0) + gzip.compress(b, 1, mtime=0) + gzip.compress(b"", 6, mtime=0) + gzip.compress(b"", 9, mtime=0) + gzip.compress(c, 9, mtime=0)
    st = check_same(hip, tmp_path, blob, FQ)
    assert st["members"] == 5 and st["slabs"] >= 3, st
    parts = [FQ[i:i + 4096] for i in range(0, len(FQ), 4096)]
    st = check_same(hip, tmp_path, b"".join(gzip.compress(x, 6, mtime=0) for x in parts), FQ)
    assert st["members"] == len(parts) and st["slabs"] >= 3, st


def test_slabs_gap_in_the_middle(hip, tmp_path, FQ, slab_1mb):
    """30 MB of 'A' inside the reads overflow every arena: the host fills that slab to its end, and the next slab starts on the device
    from the window the host uploaded"""
    text = FQ[:3_000_000] + b"A" * 30_000_000 + FQ[3_000_000:]
    st = check_same(hip, tmp_path, gzip.compress(text, 6, mtime=0), text, device_only=False)
    assert st["host_bytes"] > 0 and st["slabs"] >= 4 and st["device_bytes"] >= 3_000_000 + 1_000_000, st


def test_slabs_stored_stretch(hip, tmp_path, FQ, slab_1mb):
    """a level-0 member of 3 MB (stored blocks: no findable start) lies across slab seams between two level-6 members"""
    blob = gzip.compress(FQ[:4_000_000], 6, mtime=0) + gzip.compress(FQ[4_000_000:7_000_000], 0, mtime=0) + gzip.compress(FQ[7_000_000:], 6, mtime=0)
    st = check_same(hip, tmp_path, blob, FQ, device_only=False)
    assert st["members"] == 3 and st["slabs"] >= 3, st


def test_slabs_damage_beyond_the_first(hip, tmp_path, FQ, slab_1mb):
    z = gzip.compress(FQ, 6, mtime=0)
    assert len(z) > 3 << 20
    cases = []
    for frac in (0.6, 0.9):
        f = bytearray(z)
        f[int(len(z) * frac)] ^= 0x04
        cases.append(bytes(f))
    cases.append(z[:int(len(z) * 0.7)])
    len_bad = bytearray(z)
    len_bad[-2] ^= 0x01
    cases.append(bytes(len_bad))
    p = tmp_path / "d.gz"
    for i, blob in enumerate(cases):
        p.write_bytes(blob)
        rc_d, _, st = dev_inflate(hip, p)
        rc_h, _, _ = host_inflate(hip, p)
        assert rc_d != 0 and rc_h != 0, (i, st)
        assert st["slabs"] >= 2, (i, st)


def test_slabs_through_ingest(hip, three_files, slab_1mb, monkeypatch):
    """count_files and the read feed with the device inflater in 1 MB slabs: the oracle's histogram"""
    from jasper_amd import KmerTable
    from oracle import oracle as O
    paths, text, gz_len = three_files
    assert os.path.getsize(paths[1]) > 2 << 20
    k = 25
    db = O.OracleDB(k)
    db.count_text(text.decode())
    monkeypatch.setenv("JASPER_INGEST_GZ_DEVICE_CHUNK", str(CHUNK))
    monkeypatch.setenv("JASPER_INGEST_GZ", "device")
    t = KmerTable(k, min_slots=1 << 20)
    t.count_files(paths)
    st = t.last_inflate()
    assert t.histogram() == db.histo() and t.info()["distinct"] == db.distinct()
    assert st["slabs"] >= 3 and st["host_bytes"] == 0 and st["device_bytes"] == gz_len, st
    t.close()
    src = KmerTable(k, min_slots=1 << 16)
    dst = KmerTable(k, min_slots=1 << 20)
    src.feed_start([(p, 0, -1) for p in paths])
    while True:
        ptr, n = src.feed_next()
        if n == 0:
            break
        dst.count_bases_device(ptr, n)
        src.feed_release()
    st = src.last_inflate()
    assert dst.histogram() == db.histo() and dst.info()["distinct"] == db.distinct()
    assert st["slabs"] >= 3 and st["host_bytes"] == 0 and st["device_bytes"] == gz_len, st
    src.close()
    dst.close()
