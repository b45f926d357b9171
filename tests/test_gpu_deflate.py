"""GPU: the compressor (KmerTable.deflate_bgzf, jasper_deflate_bgzf) against the strict BGZF walker of the tests (tests/bgzf_ref.py,
held to gzip on the CPU by tests/test_bgzf_ref.py): whatever the kernel writes, zlib's raw inflate must give the text back from exactly
each member's payload, under the right CRC-32, ISIZE and BSIZE.  Nothing expected here comes from the code under test.

The texts are the smallest at which the coder can go wrong: no byte, too few bytes for a match, a block's edge, runs (distance 1, copies
that overlap themselves), repeats at the window's edge, incompressible bytes (stored blocks), every byte value, copies at the first and
the last length of every length code and distance of every distance code (the member's tokens are decoded: all 29 and all 30 must
occur, each planted copy as planted), literal frequencies whose unrestricted Huffman tree is 21 deep, and read files.  Two
bounds keep a lazy coder from passing: on random ACGT and on FASTQ the output is at most 1.03 x what zlib's Z_HUFFMAN_ONLY makes of the
same blocks (the margin: 316 code lengths sent one by one, under 300 bytes against at least 16 KiB a block, and the length limiter)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_ref

pytestmark = pytest.mark.gpu
BLOCK = 65280


@pytest.fixture(scope="module")
def table(hip):
    from jasper_amd import KmerTable
    t = KmerTable(21, min_slots=1 << 12)
    yield t
    t.close()


def fibonacci_text():
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    assert f[-1] == 17711 and sum(f) == 46367
    text = np.repeat(np.arange(65, 65 + 22, dtype=np.uint8), f)
    np.random.default_rng(21).shuffle(text)
    return text.tobytes()


TILE, HASH_BITS = 1024, 13           # deflate_gpu.hip: positions of a tile, and the bits of its hash of three bytes


def head_buckets(text):
    """the hash head every position's three bytes fall into, as deflate_gpu.hip computes it"""
    t = text.astype(np.uint32)
    return ((t[:-2] | (t[1:-1] << 8) | (t[2:] << 16)) * np.uint32(0x9E3779B1)) >> np.uint32(32 - HASH_BITS)


def copies_plan():
    """(distance, length) of the planted copies: the first and the last distance of each of the 30 distance codes, the first and the
    last length of each of the 29 length codes, short with near and long with far (a copy of 3 bytes pays only up to distance 2048)"""
    dists = sorted({d for c in range(30) for d in (bgzf_ref.DIST_BASE[c], bgzf_ref.DIST_BASE[c] + (1 << bgzf_ref.DIST_EXTRA[c]) - 1)})
    lens = sorted({n for c in range(28) for n in (bgzf_ref.LEN_BASE[c], min(bgzf_ref.LEN_BASE[c] + (1 << bgzf_ref.LEN_EXTRA[c]) - 1, 257))} | {258})
    lens = sorted(lens + [12, 20, 40, 70, 100, 150, 200][:len(dists) - len(lens)])
    assert len(dists) == len(lens) == 56
    return list(zip(dists, lens))


def copies_text():
    """random bytes with one planted copy per entry of copies_plan().  The coder finds a match through the hash head of its three bytes,
    which holds the LAST position of EARLIER tiles that fell into it, and through the byte before (distance 1).  So each copy is put where
    its source is what the coder will see: the copy begins less than `distance` bytes into a tile (its source lies in an earlier tile),
    and no position between the source and that tile falls into the source's head.  The bytes around a copy differ from those around its
    source, so the match has exactly the planted length.  What the test asserts is read from the member's decoded tokens."""
    rng = np.random.default_rng(8)
    text = rng.integers(0, 256, BLOCK, dtype=np.uint8)
    used = np.zeros(BLOCK, dtype=bool)
    planted = []

    def visible(t, p, d):
        b = head_buckets(t)
        return d == 1 or not (b[p - d + 1:p - p % TILE] == b[p - d]).any()

    for d, n in copies_plan():
        for p in range(max(d, TILE), BLOCK - n - 4):
            if d > 1 and p % TILE >= d:
                continue
            if used[p - 2:p + n + 2].any() or used[max(p - d - 2, 0):p - d + n + 2].any():
                continue
            if d > 1 and not visible(text, p, d):
                continue
            t = text.copy()
            for i in range(n):
                t[p + i] = t[p + i - d]
            if t[p + n] == t[p + n - d]:
                t[p + n] ^= 0x5A
            if t[p - 1] == t[p - 1 - d]:
                t[p - 1] ^= 0x5A
            if all(visible(t, q, e) for q, e, _ in planted + [(p, d, n)]):
                text = t
                used[p - 2:p + n + 2] = True
                used[max(p - d - 2, 0):p - d + n + 2] = True
                planted.append((p, d, n))
                break
        else:
            raise AssertionError("no place for a copy at distance %d" % d)
    return text.tobytes()


def periodic_text(period):
    rng = np.random.default_rng(period)
    text = rng.integers(0, 256, BLOCK, dtype=np.uint8)
    unit = rng.integers(0, 256, 40, dtype=np.uint8)
    for at in range(0, BLOCK - 40, period):
        text[at:at + 40] = unit
    return text.tobytes()


def synth_fastq():
    """about 2.5 MB of FASTQ from jasper_amd.synth: reads of 150 bases off a 41 kb genome with its errors and strands, as its writer
    lays them out (`@r`, the bases, `+`, 150 x `I`)"""
    from jasper_amd import synth
    rng = np.random.default_rng(5)
    reads = synth.make_reads_stream(rng, synth.make_genome(rng, 41000), 30, 150).reshape(-1, 151)[:, :150]
    rec = np.empty((len(reads), 307), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:153] = reads
    rec[:, 153:156] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 156:306] = ord("I")
    rec[:, 306] = 10
    return rec.tobytes()


def named_fastq(nreads):
    """FASTQ with what the synthetic one lacks: read names that count up, and 13 quality symbols"""
    rng = np.random.default_rng(6)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300000)]
    q = np.frombuffer(b"FFFFFFFF:F,F#", dtype=np.uint8)
    out = []
    for i in range(nreads):
        at = int(rng.integers(0, len(g) - 150))
        out.append(b"@SIM:1:FC:%d:%d 1:N:0:ACGT\n" % (i // 1000, i % 1000) + g[at:at + 150].tobytes() + b"\n+\n" + q[rng.integers(0, len(q), 150)].tobytes() + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4 * BLOCK)].tobytes()
    fq = synth_fastq()
    assert 2_400_000 < len(fq) < 2_600_000
    return {
        "empty": b"", "one": b"A", "two": b"AC", "three": b"AAA",
        "block": acgt[:BLOCK], "block_and_one": acgt[:BLOCK + 1], "blocks_and_17": acgt[:3 * BLOCK + 17],
        "run": b"G" * BLOCK,
        "period_32768": periodic_text(32768), "period_32769": periodic_text(32769),
        "random": rng.integers(0, 256, 2 * BLOCK + 100, dtype=np.uint8).tobytes(),
        "every_byte": bytes(range(256)) * 3 + bytes(reversed(range(256))),
        "copies": copies_text(),
        "fibonacci": fibonacci_text(),
        "acgt": acgt,
        "fastq": fq, "fastq_crlf": fq.replace(b"\n", b"\r\n"), "fastq_names": named_fastq(1500),
    }


def unaligned(text, shift=5):
    """the text at a pointer that is `shift` past a 16-byte boundary"""
    room = np.zeros(len(text) + 32, dtype=np.uint8)
    base = (-room.ctypes.data) % 16 + shift
    view = room[base:base + len(text)]
    view[:] = np.frombuffer(text, dtype=np.uint8)
    assert len(text) == 0 or view.ctypes.data % 16 == shift
    return view


def huffman_only(text):
    """bytes of the text's blocks under zlib's Z_HUFFMAN_ONLY, 26 bytes of member framing added to each"""
    total = 0
    for at in range(0, len(text), BLOCK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        total += len(c.compress(text[at:at + BLOCK]) + c.flush()) + 26
    return total


def deflate_checked(table, text, shift=5):
    from jasper_amd.table import deflate_bound
    out, counters, seconds = table.deflate_bgzf(unaligned(text, shift))
    blob = out.tobytes()
    parts = bgzf_ref.split(blob)
    assert b"".join(t for _, t in parts) == text
    assert [len(t) for _, t in parts] == [min(BLOCK, len(text) - at) for at in range(0, len(text), BLOCK)]      # one member per 65280 bytes, none empty
    assert all(len(m) <= 65536 and len(m) <= len(t) + 31 for m, t in parts)
    assert len(blob) <= deflate_bound(len(text)) == len(text) + 31 * len(parts)
    assert counters["blocks"] == len(parts) == counters["stored"] + counters["literal_only"] + counters["lz"]
    assert counters["stored"] == sum(1 for m, _ in parts if m[18] & 6 == 0)      # BTYPE 0
    assert (counters["matches"] > 0) == (counters["lz"] > 0) and counters["matched_bytes"] >= 3 * counters["matches"]
    assert (seconds > 0) == (len(text) > 0)
    return blob, counters


NAMES = ["empty", "one", "two", "three", "block", "block_and_one", "blocks_and_17", "run", "period_32768", "period_32769", "random", "every_byte", "copies", "fibonacci",
         "acgt", "fastq", "fastq_crlf", "fastq_names"]


@pytest.mark.parametrize("name", NAMES)
def test_members_inflate_to_the_text(table, texts, name):
    text = texts[name]
    blob, counters = deflate_checked(table, text)
    print(name, len(text), "->", len(blob), counters, "huffman-only", huffman_only(text))
    if name == "empty":
        assert blob == b"" and counters["blocks"] == 0
    if name == "random":                                # incompressible: every block stored, 31 bytes over its text
        assert counters["stored"] == counters["blocks"] == 3 and len(blob) == len(text) + 31 * 3
    if name == "run":                                   # 65280 equal bytes: runs of 258 at distance 1, a few hundred bytes
        assert counters["lz"] == 1 and counters["matched_bytes"] >= BLOCK - 300 and len(blob) < 400
    if name == "copies":                                # read from the member's own tokens: every planted copy is one match, as planted
        matches, literals, kinds = bgzf_ref.tokens(blob)
        assert kinds == [2] and counters["lz"] == 1 and counters["matches"] == len(matches)
        assert {m[0] for m in matches} == set(range(257, 286)), "a length code does not occur"
        assert {m[2] for m in matches} == set(range(30)), "a distance code does not occur"
        got = {(bgzf_ref.DIST_BASE[d] + dx, bgzf_ref.LEN_BASE[ls - 257] + lx) for ls, lx, d, dx in matches}
        assert not [c for c in copies_plan() if c not in got]      # so every code has carried its least and its most extra bits
        assert literals + sum(bgzf_ref.LEN_BASE[ls - 257] + lx for ls, lx, _, _ in matches) == len(text)
        assert counters["matched_bytes"] == len(text) - literals
    if name in ("acgt", "fastq", "fastq_crlf", "fastq_names", "fibonacci"):      # the cost rule: never more than the literals under a Huffman code
        assert len(blob) <= 1.03 * huffman_only(text), (len(blob), huffman_only(text))
    if name in ("block", "acgt"):                       # four symbols of two bits each
        assert len(blob) < 0.29 * len(text)


def test_every_alignment_and_the_text_is_left_alone(table, texts):
    text = texts["fastq"][:BLOCK + 777]
    first = None
    for shift in range(16):
        view = unaligned(text, shift)
        out, _, _ = table.deflate_bgzf(view)
        assert view.tobytes() == text
        assert bgzf_ref.members(out.tobytes()) == text
        first = out.tobytes() if first is None else first
        assert out.tobytes() == first, shift            # where the text lies changes nothing


def test_same_text_same_bytes(table, texts):
    text = texts["fastq"][:4 * BLOCK]
    a = table.deflate_bgzf(text)[0].tobytes()
    b = table.deflate_bgzf(text)[0].tobytes()
    table.deflate_bgzf(texts["copies"])                 # an unrelated call leaves other records and slots in the workspace
    table.count_bases(b"ACGTACGTTGCATGCATTTACGACGATCGATCGACTAGCTACGATCGA")
    c = table.deflate_bgzf(text)[0].tobytes()
    assert a == b == c and bgzf_ref.members(a) == text


def test_refusals_and_the_output_buffer(table, texts):
    from jasper_amd import _lib
    from jasper_amd.table import deflate_bound
    L = _lib.lib()
    assert [deflate_bound(n) for n in (0, 1, BLOCK, BLOCK + 1)] == [0, 32, BLOCK + 31, BLOCK + 1 + 62] and L.jasper_deflate_bound(-1) == -1
    nb = C.c_int64(7)
    for n in (1 << 31, 1 << 40, -1):                    # a length, not a buffer: refused before anything is looked at
        assert L.jasper_deflate_bgzf(table._h, None, n, None, 0, C.byref(nb), None, None) != 0
        assert "2^31" in L.jasper_last_error().decode() and nb.value == 0
    text = texts["random"]
    small = np.zeros(len(text), dtype=np.uint8)         # stored blocks do not fit the text's own length
    buf = np.frombuffer(text, dtype=np.uint8)
    assert L.jasper_deflate_bgzf(table._h, C.c_void_p(buf.ctypes.data), len(buf), C.c_void_p(small.ctypes.data), len(small), C.byref(nb), None, None) != 0
    assert "do not fit" in L.jasper_last_error().decode() and nb.value == 0 and not small.any()
    with pytest.raises(ValueError):
        table.deflate_bgzf(text, out=small)
    deflate_checked(table, texts["three"])              # and the workspace is as good as before
