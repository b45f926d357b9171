"""BGZF (SAM specification 4.1) on the host: the format `triobin --write-gz` writes, and the writers its bin files go through.

A BGZF file is a series of independent gzip members: the 18-byte header 1f 8b 08 04 00000000 00 ff 06 00 42 43 02 00 <member bytes - 1 as
u16>, raw deflate blocks, CRC-32 and ISIZE; at most BLOCK text bytes go into a member and at most 65536 bytes make one; the file ends with
the 28-byte empty member EOF.  Every gzip reader takes it.  compress() is the host compressor (zlib level 1): `--deflate host`, and the
baseline KmerTable.deflate_bgzf (the GPU compressor, the same blocking) is measured against.
"""
import struct
import zlib

BLOCK = 65280
MEMBER_MOST = 65536
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF = HEAD + struct.pack("<H", 27) + b"\x03\x00" + bytes(8)


def member(text, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    """one member for at most BLOCK bytes; a stored block when deflate makes them longer"""
    text = bytes(text)
    if not 0 < len(text) <= BLOCK:
        raise ValueError("a BGZF member holds 1 to %d bytes" % BLOCK)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = c.compress(text) + c.flush()
    if len(body) > len(text) + 5:
        body = b"\x01" + struct.pack("<HH", len(text), len(text) ^ 0xFFFF) + text
    return HEAD + struct.pack("<H", len(HEAD) + 2 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(text), len(text))


def compress(buf, level=1):
    """the members of buf (anything with the buffer interface), one per BLOCK bytes, without EOF; b"" for no bytes"""
    view = memoryview(buf).cast("B")
    return b"".join(member(view[at:at + BLOCK], level) for at in range(0, len(view), BLOCK))


class PlainWriter:
    """a bin file as it has always been: the bytes as they come"""

    def __init__(self, f):
        self.f, self.raw, self.written = f, 0, 0

    def write(self, arr):
        arr.tofile(self.f)
        self.raw += len(arr)
        self.written += len(arr)

    def close(self):
        self.f.close()


class BgzfWriter(PlainWriter):
    """a bin file as BGZF: every write's bytes are cut into members on their own (no tail is carried from one write to the next), close()
    ends the file with EOF.  deflate(np.uint8 array) -> the members (bytes or an array): compress, or the GPU compressor.  write_members()
    takes bytes that are members already (the _gz route calls) with the text bytes they stand for."""

    def __init__(self, f, deflate=compress):
        PlainWriter.__init__(self, f)
        self.deflate = deflate

    def write(self, arr):
        if len(arr):
            self.write_members(self.deflate(arr), len(arr))

    def write_members(self, members, raw):
        self.f.write(memoryview(members))
        self.raw += raw
        self.written += len(members)

    def close(self):
        self.f.write(EOF)
        self.written += len(EOF)
        self.f.close()
