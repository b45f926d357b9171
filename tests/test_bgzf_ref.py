"""CPU: the BGZF walker of the tests (tests/bgzf_ref.py) and the host compressor (jasper_amd/bgzf.py) held to each other and to gzip."""
import gzip
import struct

import numpy as np
import pytest

import bgzf_ref
from jasper_amd import bgzf


def texts():
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3 * bgzf.BLOCK + 17)].tobytes()
    return {"empty": b"", "one": b"A", "block": acgt[:bgzf.BLOCK], "block_and_one": acgt[:bgzf.BLOCK + 1], "blocks": acgt,
            "random": rng.integers(0, 256, bgzf.BLOCK + 5, dtype=np.uint8).tobytes(), "run": b"\x00" * (2 * bgzf.BLOCK)}


@pytest.mark.parametrize("name", sorted(texts()))
def test_host_compressor_writes_what_gzip_and_the_walker_read(name):
    text = texts()[name]
    blob = bgzf.compress(text) + bgzf.EOF
    assert gzip.decompress(blob) == text
    assert bgzf_ref.walk(blob) == text
    parts = bgzf_ref.split(blob[:-28])
    assert len(parts) == -(-len(text) // bgzf.BLOCK)            # one member per 65280 bytes
    assert all(len(m) <= len(t) + 31 for m, t in parts)
    assert bgzf.compress(np.frombuffer(text, dtype=np.uint8)) == blob[:-28]      # an array goes in as bytes do
    assert bgzf.EOF == bgzf_ref.EOF_MARKER and len(bgzf.EOF) == 28 and gzip.decompress(bgzf.EOF) == b""


def test_random_bytes_are_stored():
    text = texts()["random"]
    (m0, t0), (m1, t1) = bgzf_ref.split(bgzf.compress(text))
    assert len(m0) == len(t0) + 31 and m0[18] == 1 and len(m1) <= len(t1) + 31      # (five bytes are shorter under the fixed code)


def test_walker_refuses_damaged_files():
    text = texts()["blocks"]
    good = bgzf.compress(text) + bgzf.EOF
    first = struct.unpack_from("<H", good, 16)[0] + 1

    def damaged(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)

    cases = {
        "BSIZE one too many": damaged(16, (good[16] + 1) & 0xFF),
        "BSIZE one too few": damaged(16, (good[16] - 1) & 0xFF),
        "no end marker": good[:-28],
        "half an end marker": good[:-14],
        "a flipped CRC bit": damaged(first - 8, good[first - 8] ^ 1),
        "a wrong ISIZE": damaged(first - 4, good[first - 4] ^ 1),
        "a wrong header byte": damaged(3, 0),
        "an empty member inside": good[:first] + bgzf.EOF + good[first:],
        "a flipped payload bit": damaged(first - 20, good[first - 20] ^ 0x10),
        "bytes behind the marker": good + b"\x00",
    }
    for what, blob in cases.items():
        with pytest.raises(bgzf_ref.Bad):
            bgzf_ref.walk(blob)
            pytest.fail("the walker takes a file with " + what)
    long_member = bytearray(bgzf.member(b"A" * 100))            # ISIZE above 65280 cannot be built with member(); too long a text can
    with pytest.raises(ValueError):
        bgzf.member(b"A" * (bgzf.BLOCK + 1))
    assert bgzf_ref.members(bytes(long_member)) == b"A" * 100
    with pytest.raises(bgzf_ref.Bad):
        bgzf_ref.members(bgzf.EOF)                               # a compressor's output holds no empty member
