"""A strict BGZF walker (SAM specification 4.1), written against the specification and zlib's raw inflate alone: what the tests hold every
BGZF producer of the project to -- jasper_amd/bgzf.py on the host, KmerTable.deflate_bgzf and the _gz route calls on the GPU.

members(blob) walks a series of members WITHOUT the end marker (what the compressors return), walk(blob) a whole file (members, then the
28-byte empty member, and no other empty member); both return the text and raise Bad with what is wrong.
"""
import struct
import zlib

HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF_MARKER = HEAD + bytes([0x1b, 0x00, 0x03, 0x00]) + bytes(8)
MEMBER_MOST = 65536
TEXT_MOST = 65280


class Bad(Exception):
    pass


def split(blob):
    """-> [(member bytes, its text)]; every check of one member is here"""
    blob = bytes(blob)
    out, at = [], 0
    while at < len(blob):
        if len(blob) - at < 26:
            raise Bad("%d bytes at %d are too few for a member" % (len(blob) - at, at))
        if blob[at:at + 16] != HEAD:
            raise Bad("the member at %d does not begin with the BGZF header" % at)
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        if size < 26 or at + size > len(blob):
            raise Bad("the member at %d: BSIZE says %d bytes, %d are left" % (at, size, len(blob) - at))
        if size > MEMBER_MOST:
            raise Bad("the member at %d has %d bytes" % (at, size))
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(blob[at + 18:at + size - 8])
        except zlib.error as e:
            raise Bad("the member at %d: %s" % (at, e))
        if not d.eof or d.unused_data or d.unconsumed_tail:
            raise Bad("the member at %d: its deflate data ends %s its payload" % (at, "before the end of" if d.eof else "after"))
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        if isize != len(text) or isize > TEXT_MOST:
            raise Bad("the member at %d: ISIZE %d, %d bytes of text" % (at, isize, len(text)))
        if crc != zlib.crc32(text):
            raise Bad("the member at %d: CRC-32 %08x, its text has %08x" % (at, crc, zlib.crc32(text)))
        out.append((blob[at:at + size], text))
        at += size
    return out


def members(blob):
    """a series of members without the end marker and without an empty member -> the text"""
    parts = split(blob)
    if any(not t for _, t in parts):
        raise Bad("an empty member among the members")
    return b"".join(t for _, t in parts)


def walk(blob):
    """a whole BGZF file -> the text"""
    blob = bytes(blob)
    if blob[-28:] != EOF_MARKER:
        raise Bad("the file does not end with the 28-byte empty member")
    return members(blob[:-28])


# ---- the tokens of a member: a symbol-level inflate written from RFC 1951, for tests that ask WHICH codes a compressor used ----------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lengths):
    """canonical Huffman code of the lengths -> {(length, code): symbol}"""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for sym, ln in enumerate(lengths):
        if ln:
            table[(ln, nxt[ln])] = sym
            nxt[ln] += 1
    return table


def _symbol(bits, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise Bad("a code of more than 15 bits")


def tokens(member):
    """one member -> [(length symbol 257..285, extra, distance symbol 0..29, extra) per match], its literals, and the block types met"""
    bits, matches, literals, kinds = _Bits(bytes(member)[18:-8]), [], 0, []
    while True:
        final, kind = bits.take(1), bits.take(2)
        kinds.append(kind)
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n = bits.take(16)
            if bits.take(16) != n ^ 0xFFFF:
                raise Bad("a stored block's lengths")
            bits.pos += 8 * n
            literals += n
        elif kind in (1, 2):
            if kind == 1:
                ll, dd = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits.take(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                ll, dd = lens[:hlit], lens[hlit:hlit + hdist]
            lt, dt = _decoder(ll), _decoder(dd)
            while True:
                s = _symbol(bits, lt)
                if s < 256:
                    literals += 1
                elif s == 256:
                    break
                else:
                    ex = bits.take(LEN_EXTRA[s - 257])
                    d = _symbol(bits, dt)
                    matches.append((s, ex, d, bits.take(DIST_EXTRA[d])))
        else:
            raise Bad("block type 3")
        if final:
            return matches, literals, kinds
