"""Helpers of tests/test_deflate_writer.py and tests/test_gpu_inflate_streams.py: a bit-level writer of deflate (RFC 1951) and gzip
(RFC 1952) streams driven by token lists, for streams that zlib's deflate never writes, and for streams that are wrong on purpose.

A token is
    an int 0..255                    a literal byte
    (length, distance)               a match; length 258 is written as symbol 285
    (length, distance, 284)          the same with the length symbol chosen: 258 as symbol 284 plus extra 31
    ("lit", symbol)                  a raw literal/length symbol of the block's code, no extra bits (286, 287, or a length without a distance)
    ("dist", symbol)                 a raw distance symbol of the block's code, no extra bits (30, 31)
    ("bits", value, n)               n raw bits, least significant first
`expected_text` interprets a token list on its own: it shares no code with the writer and none with zlib.  Raw tokens have no text.
The writer checks only what the caller says is meant to hold (`complete=`): everything else is written as asked.
"""
import zlib

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
FEXTRA, FNAME, FCOMMENT, FHCRC = 4, 8, 16, 2


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        """zero bits up to the next byte boundary; how many there were"""
        pad = (8 - self.n) & 7
        self.bits(0, pad)
        return pad

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def bitlen(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def kraft(lengths):
    """sum of 2^-len over the used codes, in units of 2^-15: a complete code gives 32768"""
    return sum(1 << (15 - l) for l in lengths if l)


def canonical(lengths):
    """symbol -> (code already bit-reversed for an LSB-first writer, length), the canonical assignment of RFC 1951 3.2.2.  For an
    over-subscribed set the codes overflow their lengths and are cut to them: such a block is wrong anyway."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def kraft_fill(n, preset):
    """n code lengths: `preset` (symbol -> length) kept, the other symbols given two adjacent lengths (the shorter to the lower
    symbols) so that the code is complete"""
    free = [s for s in range(n) if s not in preset]
    rest = 32768 - kraft(preset.values())
    m = len(free)
    for L in range(1, 15):
        unit = 1 << (14 - L)
        if rest % unit == 0 and 0 <= rest // unit - m <= m:
            a = rest // unit - m
            lens = [0] * n
            for s, l in preset.items():
                lens[s] = l
            for i, s in enumerate(free):
                lens[s] = L if i < a else L + 1
            assert kraft(lens) == 32768
            return lens
    raise ValueError("no two adjacent lengths complete this code")


def rle(lens):
    """code lengths -> code-length-code symbols: an int 0..15, (16, n) the previous length n = 3..6 more times, (17, n) n = 3..10
    zeros, (18, n) n = 11..138 zeros"""
    out = []
    i = 0
    while i < len(lens):
        v = lens[i]
        j = i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [0] * run
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [v] * run
        i = j
    return out


def _balanced(symbols):
    """a complete code over these symbols (at least two), lengths differing by at most one"""
    syms = sorted(symbols)
    n = len(syms)
    k = max(1, (n - 1).bit_length())
    short = (1 << k) - n
    return {s: (k - 1 if i < short else k) for i, s in enumerate(syms)}


def _length_symbol(length, lsym):
    if lsym is not None:
        li = lsym - 257
        assert 0 <= length - LBASE[li] < (1 << LEXT[li])
        return li
    if length == 258:
        return 28
    li = max(i for i in range(28) if LBASE[i] <= length)
    assert length - LBASE[li] < (1 << LEXT[li])
    return li


class Deflate:
    """one raw deflate stream, block by block; .tokens is everything written so far as literal and match tokens"""

    def __init__(self):
        self.w = BitWriter()
        self.tokens = []

    def bitlen(self):
        return self.w.bitlen()

    def finish(self):
        return self.w.getvalue()

    def stored(self, data=b"", final=False, nlen=None):
        """a stored block of 0..65535 bytes; nlen: the complement field as written (default: the right one).  Returns the number of
        padding bits between the block header and LEN."""
        assert len(data) <= 65535
        self.w.bits(1 if final else 0, 1)
        self.w.bits(0, 2)
        pad = self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(data)
        self.tokens += list(data)
        return pad

    def reserved(self, final=False):
        """a block header with BTYPE = 3"""
        self.w.bits(1 if final else 0, 1)
        self.w.bits(3, 2)

    def _symbols(self, tokens, ll, dd):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.bits(*ll[t])
            elif t[0] == "lit":
                w.bits(*ll[t[1]])
            elif t[0] == "dist":
                w.bits(*dd[t[1]])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                length, dist = t[0], t[1]
                li = _length_symbol(length, t[2] if len(t) > 2 else None)
                w.bits(*ll[257 + li])
                w.bits(length - LBASE[li], LEXT[li])
                di = max(i for i in range(30) if DBASE[i] <= dist)
                assert dist - DBASE[di] < (1 << DEXT[di])
                w.bits(*dd[di])
                w.bits(dist - DBASE[di], DEXT[di])
        self.tokens += tokens

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        ll = canonical(FIXED_LL)
        self._symbols(tokens, ll, canonical(FIXED_D))
        if eob:
            self.w.bits(*ll[256])

    def dynamic(self, tokens, ll_lens, d_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_syms=None,
                complete=(True, True), eob=True):
        """a dynamic block.  ll_lens / d_lens: code lengths of the literal/length and distance symbols (shorter lists are padded with
        zeros up to hlit / hdist, which default to the lists' lengths, at least 257 and 1).  complete: which of the two codes are
        meant to be complete -- asserted.  cl_syms: the code-length-code symbols as rle() gives them, written as they are, whatever
        they add up to (default: rle of the hlit + hdist lengths as one sequence).  cl_lens: symbol -> length of the code-length code
        (default: a complete code over the symbols used); hclen: how many of them are written (default: up to the last used)."""
        hlit = max(257, len(ll_lens)) if hlit is None else hlit
        hdist = max(1, len(d_lens)) if hdist is None else hdist
        ll_lens = list(ll_lens) + [0] * (hlit - len(ll_lens))
        d_lens = list(d_lens) + [0] * (hdist - len(d_lens))
        if complete[0]:
            assert kraft(ll_lens) == 32768
        if complete[1]:
            assert kraft(d_lens) == 32768
        if cl_syms is None:
            cl_syms = rle(ll_lens[:hlit] + d_lens[:hdist])
        used = {s if isinstance(s, int) else s[0] for s in cl_syms}
        if cl_lens is None:
            if len(used) == 1:
                used = used | {min({0, 1} - used)}
            cl_lens = _balanced(used)
            assert kraft(cl_lens.values()) == 32768
        if hclen is None:
            hclen = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl_lens.get(s, 0)))
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens.get(s, 0), 3)
        cl = canonical([cl_lens.get(s, 0) for s in range(19)])
        for s in cl_syms:
            if isinstance(s, int):
                w.bits(*cl[s])
            else:
                w.bits(*cl[s[0]])
                w.bits(s[1] - (3, 3, 11)[s[0] - 16], (2, 3, 7)[s[0] - 16])
        ll = canonical(ll_lens)
        self._symbols(tokens, ll, canonical(d_lens))
        if eob:
            w.bits(*ll[256])


def expected_text(tokens, history=b""):
    """the text of a token list: literals and copies, nothing else.  history: text that a match may reach into (not returned)"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if isinstance(t[0], str):
            raise ValueError("a raw token has no text")
        length, dist = t[0], t[1]
        if not (3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out)):
            raise ValueError("match out of range")
        for _ in range(length):
            out.append(out[-dist])
    return bytes(out[len(history):])


def gzip_member(deflate_bytes, text, flags=0, crc=None, isize=None, extra=b"AB\x02\x00xy", name=b"reads.fq", comment=b"a comment"):
    """one RFC 1952 member around a raw deflate stream.  flags: FEXTRA | FNAME | FCOMMENT | FHCRC; crc / isize: the trailer as
    written (default: those of text)"""
    hdr = b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\x03"
    if flags & FEXTRA:
        hdr += len(extra).to_bytes(2, "little") + extra
    if flags & FNAME:
        hdr += name + b"\0"
    if flags & FCOMMENT:
        hdr += comment + b"\0"
    if flags & FHCRC:
        hdr += (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little")
    crc = zlib.crc32(text) if crc is None else crc
    isize = len(text) if isize is None else isize
    return hdr + deflate_bytes + (crc & 0xFFFFFFFF).to_bytes(4, "little") + (isize & 0xFFFFFFFF).to_bytes(4, "little")


def gzip_stream(members):
    return b"".join(members)
