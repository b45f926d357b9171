"""CPU: the crafted deflate / gzip streams of tests/test_gpu_inflate_streams.py, pinned against zlib.

CASES is the one table: name -> (blob, expected text, or None where the stream is wrong).  For a valid case zlib must give exactly
the text that deflate_writer.expected_text (an interpreter that owes nothing to zlib) gives for the token list; for a wrong one zlib
must refuse it, with the complaint tabled in REFUSED -- so the verdicts the device inflater is held to are zlib's, and a wrong
stream is refused for the reason it was built for, not because of its checksum.  DEVICE names the cases whose every decoder of the
device inflater (4096 compressed bytes each, an arena of 16 * 4096 symbols) must hold its text: their sizes are checked here.
"""
import gzip
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from test_gpu_inflate import fastq_text            # (the read text of that module's FQ fixture; importing it needs no GPU)
from deflate_writer import Deflate, gzip_member

CHUNK = 4096                      # the smallest decoder chunk the library allows
CAP = 16 * CHUNK                  # symbols one decoder's arena holds

FLAT_LL = [8] * 226 + [9] * 60    # a complete near-flat code over all 286 literal/length symbols
FLAT_D = [4, 4] + [5] * 28        # ... and over all 30 distance symbols
assert dw.kraft(FLAT_LL) == 32768 and dw.kraft(FLAT_D) == 32768

CASES = {}
DEVICE = set()                    # cases the device must decode without the host's help
REFUSED = {}                      # wrong case -> what zlib says
LENIENT = set()                   # wrong cases whose trailer is that of the text a decoder WITHOUT the check would give
MEMBERS = {}                      # valid case -> gzip members in it (default 1)


def flat(d, rng, nlit, head=(), final=False, hi=256):
    """one dynamic block under the flat code: the tokens of `head`, then nlit random literals"""
    d.dynamic(list(head) + [int(x) for x in rng.integers(0, hi, nlit)], FLAT_LL, FLAT_D, final=final)


def one_member(d, **kw):
    return gzip_member(d.finish(), dw.expected_text(d.tokens), **kw), dw.expected_text(d.tokens)


def add(name, blob, text, device=False, members=1):
    assert name not in CASES
    CASES[name] = (blob, text)
    if device:
        DEVICE.add(name)
    MEMBERS[name] = members


def wrong(name, blob, says):
    assert name not in CASES
    CASES[name] = (blob, None)
    REFUSED[name] = says


# ---- valid streams ----------------------------------------------------------------------------------------------------------------
# the matches every far_matches block begins with once 32 KB of text exist: the window's two ends (32768, 32767), zlib's limit + 1
# (32507), then copies of what those just wrote -- run lengths 1 and 7, a 16-byte copy (distance 300), a period of 3, and a match
# that starts one byte before the block (distance = bytes written + 1)
FAR_HEAD = [(258, 32768), (258, 32767, 284), (3, 32507), (258, 1), (9, 7), (40, 300), (11, 3)]
FAR_HEAD = FAR_HEAD + [(6, sum(t[0] for t in FAR_HEAD) + 1)]


def build_far_matches():
    d, rng = Deflate(), np.random.default_rng(5)
    n = 0
    for i in range(40):
        head = FAR_HEAD if n >= 32768 else []
        flat(d, rng, 3600, head, final=i == 39)
        n += 3600 + sum(t[0] for t in head)
    add("far_matches", *one_member(d), device=True)


# literal/length code: 24 symbols of 11..15 bits (past the 10-bit table), among them the end-of-block code's neighbours 284 and 285
LONG_LL = {285: 15, 284: 15, 270: 15, 260: 15, 0: 15, 1: 15, 2: 15, 3: 15, 257: 14, 258: 14, 4: 14, 5: 14, 269: 13, 280: 13, 6: 13, 7: 13,
           265: 12, 275: 12, 8: 12, 9: 12, 281: 11, 279: 11, 10: 11, 11: 11}
# distance code: symbols 22..29 of 9..15 bits (past the 8-bit table)
LONG_D = {29: 15, 28: 15, 27: 14, 26: 13, 25: 12, 24: 11, 23: 10, 22: 9, 21: 8, 20: 7, 19: 6, 18: 5}
LONG_MATCHES = [(258, 32768), (258, 16385, 284), (23, 12289), (6, 8193), (3, 6145), (4, 4097), (19, 3073), (115, 2049), (11, 32768),
                (51, 24577), (131, 20000), (99, 9), (258, 3)]


def build_long_codes():
    d, rng = Deflate(), np.random.default_rng(6)
    ll, dd = dw.kraft_fill(286, LONG_LL), dw.kraft_fill(30, LONG_D)
    assert sorted(set(ll)) == [8, 9, 11, 12, 13, 14, 15] and max(dd[:22]) <= 8
    for _ in range(10):
        flat(d, rng, 3600)
    for _ in range(2):
        toks = []
        for m in LONG_MATCHES:
            toks += [int(x) for x in rng.integers(0, 12, 12)] + [m] + [int(x) for x in rng.integers(0, 256, 20)]
        toks += list(range(12))
        used_l = {t if isinstance(t, int) else 257 + dw._length_symbol(t[0], t[2] if len(t) > 2 else None) for t in toks}
        used_d = {max(i for i in range(30) if dw.DBASE[i] <= t[1]) for t in toks if not isinstance(t, int)}
        assert all(s in used_l for s in LONG_LL) and all(s in used_d for s in range(22, 30))
        d.dynamic(toks, ll, dd)
        flat(d, rng, 3600)
    d.stored(b"", final=True)
    add("long_codes", *one_member(d), device=True)


def build_small_tables():
    rng = np.random.default_rng(7)
    # a distance code of one code of one bit (its other code is unused): distance symbol 0, then symbol 4 (distance 5..6)
    d = Deflate()
    flat(d, rng, 3000)
    d.dynamic([65, 66, 67, (10, 1), 68, (258, 1), 69], FLAT_LL, [1], complete=(True, False))
    d.dynamic([70, 71, 72, 73, 74, 75, (30, 5), (7, 6)], FLAT_LL, [0, 0, 0, 0, 1], complete=(True, False))
    flat(d, rng, 3000, final=True)
    add("single_distance_code", *one_member(d), device=True)
    # no distance code at all: HDIST = 1, its one length 0
    d = Deflate()
    flat(d, rng, 3000)
    d.dynamic([int(x) for x in rng.integers(0, 256, 500)], FLAT_LL, [0], complete=(True, False))
    flat(d, rng, 3000, [(20, 3100)], final=True)
    add("empty_distance_code", *one_member(d), device=True)
    # a literal/length code that is the end-of-block code alone, one bit long
    d = Deflate()
    flat(d, rng, 3000)
    d.dynamic([], [0] * 256 + [1], [0], complete=(False, False))
    d.dynamic([], [0] * 256 + [1], [0], complete=(False, False))
    flat(d, rng, 3000, [(20, 3000)], final=True)
    add("eob_only_block", *one_member(d), device=True)


def build_hlit_hdist_max():
    rng = np.random.default_rng(8)
    d = Deflate()
    flat(d, rng, 3000)
    # HLIT = 286, HDIST = 30, all 19 code-length-code lengths sent (15 is the last in their order); one repeat code 16 runs over the
    # last two literal/length lengths into the first four distance lengths
    ll = dw.kraft_fill(286, {283: 5, 284: 5, 285: 5, 0: 15, 1: 15, 2: 14, 3: 13, 4: 12, 5: 11, 6: 10})
    dd = [5] * 28 + [4, 4]
    syms = dw.rle(ll[:283]) + [5, (16, 6)] + dw.rle(dd[4:])
    toks = [int(x) for x in rng.integers(0, 256, 400)] + [(258, 1), (258, 2, 284), (200, 3000), (3, 17)]
    d.dynamic(toks, ll, dd, hlit=286, hdist=30, hclen=19, cl_syms=syms)
    # the fewest code-length-code lengths that can say anything but 0: five (16, 17, 18, 0, 8).  Lengths 8 and 0 only; repeat codes 16
    # copy a 0 from the literal/length lengths into all 30 distance lengths
    ll = [8] * 255 + [0, 8] + [0] * 29
    syms = [8] + [(16, 6)] * 42 + [8, 8, 0, 8, 0] + [(16, 6)] * 9 + [(16, 4)]
    d.dynamic([int(x) for x in rng.integers(0, 255, 400)], ll, [0] * 30, hlit=286, hdist=30, hclen=5, cl_syms=syms, cl_lens={16: 1, 0: 2, 8: 2},
              complete=(True, False))
    flat(d, rng, 3000, [(100, 3500)], final=True)
    add("hlit_hdist_max", *one_member(d), device=True)


def build_stored():
    rng = np.random.default_rng(9)
    pads = set()
    for want in range(8):
        d = Deflate()
        flat(d, rng, 200)
        # a fixed block of 3 + 8 * 20 + k + 7 bits: k of its literals have 9-bit codes, chosen for `want` padding bits after the
        # stored block's 3 header bits
        k = -(d.bitlen() + 173 + want) % 8
        d.fixed([65 + i for i in range(20 - k)] + [200 + i for i in range(k)])
        pad = d.stored(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
        pads.add(pad)
        assert d.stored(b"") == 5                                   # an empty stored block in the middle (a flush marker)
        d.fixed([(30, 300), 66, 67])
        d.stored(b"between")
        flat(d, rng, 100, [(258, 400)])
        d.stored(b"", final=True)                                   # ... and as the last block
        add("stored_align_pad%d" % pad, *one_member(d), device=True)
    assert pads == set(range(8))
    # a full-size stored block: with the one literal before it, exactly one decoder's arena; the block after it is the first
    # findable start behind it (the stored bytes are all 0xFF: no bit pattern in them starts a dynamic block or a member)
    d = Deflate()
    d.fixed([65])
    d.stored(b"\xff" * 65535)
    flat(d, rng, 3000, [(258, 32768), (258, 1)])
    flat(d, rng, 3000, final=True)
    add("stored_65535", *one_member(d), device=True)


def build_zlib_streams():
    fq = fastq_text(1, 9_000)                   # ~3 MB
    for name, mode in (("flush_markers_sync", zlib.Z_SYNC_FLUSH), ("flush_markers_full", zlib.Z_FULL_FLUSH)):
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        blob = b"".join(co.compress(fq[i:i + 32768]) + co.flush(mode) for i in range(0, len(fq), 32768)) + co.flush()
        assert blob.count(b"\x00\x00\xff\xff") >= len(fq) // 32768
        add(name, blob, fq, device=True)
    # memLevel 1: blocks of 128 symbols, many of them fixed; memLevel 9: blocks of up to 65535 symbols, more text than one decoder's
    # arena holds at this chunk size, so those two are not DEVICE cases (the device gives such a block to the host)
    text = fq[:1_000_000]
    for wbits in (9, 12):
        for mem in (1, 9):
            co = zlib.compressobj(6, zlib.DEFLATED, 16 + wbits, mem)
            add("zlib_wbits%d_mem%d" % (wbits, mem), co.compress(text) + co.flush(), text, device=mem == 1)
    # a .gz inside a .gz: the outer stream is stored blocks, and every member header and dynamic header of the inner stream lies in
    # them as a candidate start that decodes cleanly and is false
    rng = np.random.default_rng(10)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2_000_000)].tobytes()
    inner = gzip.compress(bases, 6, mtime=0)
    add("nested_gzip", gzip.compress(inner, 6, mtime=0), inner)
    inner = b"".join(gzip.compress(bases[i:i + 4096], 6, mtime=0) for i in range(0, len(bases), 4096))
    add("nested_gzip_4k_members", gzip.compress(inner, 0, mtime=0), inner)     # (level 0: deflate would find the repeated headers worth coding)
    for n in ("nested_gzip", "nested_gzip_4k_members"):
        assert len(CASES[n][0]) > len(CASES[n][1]) and CASES[n][1][100_000:100_040] in CASES[n][0]     # the outer stream is stored blocks
    # more member ends than one decoder records
    a, b = fq[:50_000], fq[50_000:90_000]
    add("many_member_ends_200_empty", gzip.compress(a, 6, mtime=0) + gzip.compress(b"", 6, mtime=0) * 200 + gzip.compress(b, 6, mtime=0), a + b, members=202)
    add("many_member_ends_3000_small", b"".join(gzip.compress(fq[40 * i:40 * i + 40], 6, mtime=0) for i in range(3000)), fq[:120_000], members=3000)


# ---- wrong streams -------------------------------------------------------------------------------------------------------------
# Every wrong block stands between two good ones, the second of them the member's last, and the member has a real trailer: a decoder
# that lacks the check meets no run of zero bytes or missing trailer that would refuse the file for it.  Where such a decoder's text
# is well defined (LENIENT), the trailer's CRC-32 and ISIZE are those of that text: then nothing but the check itself can refuse
# the file.  Elsewhere (a code that cannot be assigned, a symbol that stands for nothing) the trailer is that of the good tokens.
def readable(tokens):
    return [t for t in tokens if isinstance(t, int) or not isinstance(t[0], str)]


def wrong_block(name, says, write, lenient=None):
    rng = np.random.default_rng(11)
    d = Deflate()
    flat(d, rng, 300)
    write(d)
    flat(d, rng, 50, final=True)
    if lenient:
        LENIENT.add(name)
    text = lenient(d.tokens) if lenient else dw.expected_text(readable(d.tokens))
    wrong(name, gzip_member(d.finish(), text), says)


def build_wrong():
    lit = [72, 101, 108, 108, 111]
    as_written = dw.expected_text          # the lenient text: the tokens as they were written
    # the three code kinds, over-subscribed (no codes can be assigned: no lenient text) and incomplete (the canonical codes exist)
    wrong_block("oversubscribed_code_length_code", "invalid code lengths set", lambda d: d.dynamic(lit, FLAT_LL, FLAT_D, cl_lens={0: 1, 4: 2, 5: 2, 8: 2, 9: 2, 16: 3, 17: 3, 18: 3}))
    wrong_block("incomplete_code_length_code", "invalid code lengths set", lambda d: d.dynamic(lit, FLAT_LL, FLAT_D, cl_lens={4: 2, 5: 2, 8: 2, 9: 3, 16: 4}), as_written)
    wrong_block("oversubscribed_literal_code", "invalid literal/lengths set", lambda d: d.dynamic(lit, [7] + FLAT_LL[1:], FLAT_D, complete=(False, True)))
    wrong_block("incomplete_literal_code", "invalid literal/lengths set", lambda d: d.dynamic(lit, [9] + FLAT_LL[1:], FLAT_D, complete=(False, True)), as_written)
    wrong_block("oversubscribed_distance_code", "invalid distances set", lambda d: d.dynamic(lit, FLAT_LL, [3] + FLAT_D[1:], complete=(True, False)))
    wrong_block("incomplete_distance_code", "invalid distances set", lambda d: d.dynamic(lit + [(5, 1), (4, 2)], FLAT_LL, [2, 2], complete=(True, False)), as_written)
    wrong_block("no_end_of_block_code", "missing end-of-block", lambda d: d.dynamic(lit, [8] * 226 + [9] * 30 + [0, 8] + [9] * 28, FLAT_D, eob=False))
    # a repeat of "the previous length" with nothing before it: lenient decoders take 0 (the code is complete with three zeros in front)
    ll0 = dw.kraft_fill(286, {0: 0, 1: 0, 2: 0})
    wrong_block("repeat_16_at_position_0", "invalid bit length repeat", lambda d: d.dynamic(lit, ll0, FLAT_D, cl_syms=[(16, 3)] + dw.rle(ll0[3:] + FLAT_D)), as_written)
    # a run three lengths past the last one: lenient decoders drop the excess
    wrong_block("run_past_hlit_plus_hdist", "invalid bit length repeat", lambda d: d.dynamic(lit, FLAT_LL, FLAT_D, cl_syms=dw.rle(FLAT_LL + FLAT_D[:27]) + [(16, 6)]), as_written)
    wrong_block("hlit_287", "too many length or distance symbols", lambda d: d.dynamic(lit, FLAT_LL + [0], FLAT_D, hlit=287), as_written)
    wrong_block("hdist_31", "too many length or distance symbols", lambda d: d.dynamic(lit, FLAT_LL, FLAT_D + [0], hdist=31), as_written)
    wrong_block("hclen_4_says_only_zero_lengths_zlib_refuses", "missing end-of-block",
                lambda d: d.dynamic(lit, FLAT_LL, FLAT_D, hclen=4, cl_lens={18: 1, 17: 2, 0: 2}, cl_syms=[(18, 138), (18, 138), (18, 40)], complete=(True, True)))
    for s in (286, 287):
        wrong_block("literal_length_symbol_%d" % s, "invalid literal/length code", lambda d: d.fixed(lit + [("lit", s)] + lit))
    for s in (30, 31):
        wrong_block("distance_symbol_%d" % s, "invalid distance code", lambda d: d.fixed(lit + [("lit", 257), ("dist", s)] + lit))
    wrong_block("distance_with_empty_distance_code", "invalid distance code", lambda d: d.dynamic(lit + [("lit", 257), ("bits", 0, 5)] + lit, FLAT_LL, [0], complete=(True, False)))
    wrong_block("unused_code_of_single_distance_code", "invalid distance code", lambda d: d.dynamic(lit + [("lit", 257), ("bits", 1, 1)] + lit, FLAT_LL, [1], complete=(True, False)))
    wrong_block("block_type_3", "invalid block type", lambda d: d.reserved())
    wrong_block("stored_nlen_mismatch", "invalid stored block lengths", lambda d: d.stored(b"stored text", nlen=(~11 & 0xFFFF) ^ 0x0100), as_written)
    # a reference before the member's start: at output position < distance in the first member (a lenient decoder reads its zeroed window)
    wrong_block("too_far_back_first_member", "invalid distance too far back", lambda d: d.fixed([(10, 400)] + lit),
                lenient=lambda t: dw.expected_text(t, bytes(32768)))
    # ... and in a second member, into the first member's text (which is what a lenient decoder reads)
    rng = np.random.default_rng(12)
    d1, d2 = Deflate(), Deflate()
    flat(d1, rng, 500, final=True)
    flat(d2, rng, 100)
    d2.fixed([(10, 300)] + lit)
    flat(d2, rng, 50, final=True)
    t1 = dw.expected_text(d1.tokens)
    wrong("too_far_back_second_member", gzip_member(d1.finish(), t1) + gzip_member(d2.finish(), dw.expected_text(d2.tokens, t1)), "invalid distance too far back")
    LENIENT.add("too_far_back_second_member")


def chunk_start_pair(dist):
    """member 1, then member 2 = a block of 100 bytes and a block B that begins with a match `dist` back.  The layout puts the one
    nominal cut (header + 4096) inside the 100-byte block and keeps the file under two chunks, so B is the only block boundary a
    second decoder can start at: two accepted chunks mean that B was one.  dist = 200 reaches into member 1 and is seen only when B's
    symbols are resolved against the window."""
    for n1 in range(3700, 4000, 5):
        rng = np.random.default_rng(13)
        d1, d2 = Deflate(), Deflate()
        flat(d1, rng, n1, final=True)
        t1 = dw.expected_text(d1.tokens)
        m1 = gzip_member(d1.finish(), t1)
        flat(d2, rng, 100)
        b_bit = 8 * (len(m1) + 10) + d2.bitlen()
        flat(d2, rng, 3000, [(20, dist)])                          # (not the last block: the start search skips those)
        d2.stored(b"", final=True)
        t2 = dw.expected_text(d2.tokens, t1)
        blob = m1 + gzip_member(d2.finish(), t2)
        cut = 10 + CHUNK
        if len(m1) + 10 + 60 < cut and b_bit >= 8 * cut + 64 and len(blob) <= cut + CHUNK:
            return blob, t1 + t2
    raise AssertionError("no layout")


def build_all():
    build_far_matches()
    build_long_codes()
    build_small_tables()
    build_hlit_hdist_max()
    build_stored()
    build_zlib_streams()
    build_wrong()
    add("chunk_start_twin_distance_50", *chunk_start_pair(50), device=True, members=2)
    wrong("too_far_back_at_chunk_start", chunk_start_pair(200)[0], "invalid distance too far back")
    LENIENT.add("too_far_back_at_chunk_start")


build_all()
VALID = sorted(n for n, (_, t) in CASES.items() if t is not None)
WRONG = sorted(n for n, (_, t) in CASES.items() if t is None)


def zlib_inflate(blob):
    """every member of a gzip file through zlib; what zlib raises, or a truncated stream, is an error"""
    out = []
    n = 0
    while blob:
        d = zlib.decompressobj(31)
        out.append(d.decompress(blob))
        if not d.eof:
            raise zlib.error("truncated")
        blob = d.unused_data.lstrip(b"\0")
        n += 1
    return b"".join(out), n


# ---- the writer itself ------------------------------------------------------------------------------------------------------------
def test_writer_pieces():
    assert dw.kraft(dw.FIXED_LL) == 32768 and dw.kraft(dw.FIXED_D) == 32768
    assert dw.canonical([2, 1, 3, 3]) == {0: (0b01, 2), 1: (0b0, 1), 2: (0b011, 3), 3: (0b111, 3)}      # RFC 1951 3.2.2, bit-reversed
    assert dw.rle([0] * 150 + [7] * 9 + [0, 0] + [3]) == [(18, 138), (18, 12), 7, (16, 6), 7, 7, 0, 0, 3]
    assert dw.expected_text([97, 98, (5, 2), (3, 7)]) == b"abababaaba"
    assert dw.expected_text([(4, 2)], b"xy") == b"xyxy"
    with pytest.raises(ValueError):
        dw.expected_text([97, (3, 2)])
    lens = dw.kraft_fill(30, LONG_D)
    assert dw.kraft(lens) == 32768 and lens[29] == 15 and lens[:18] == [4] * 12 + [5] * 6
    with pytest.raises(ValueError):
        dw.kraft_fill(30, {29: 15, 28: 15})
    # fixed and stored blocks, both spellings of length 258, every header flag
    d = Deflate()
    d.fixed([120] * 10 + [(258, 10), (258, 1, 284), (3, 1), 200, 255])
    d.stored(b"stored")
    d.stored(b"", final=True)
    text = dw.expected_text(d.tokens)
    assert zlib.decompress(d.finish(), -15) == text and len(text) == 10 + 258 + 258 + 3 + 2 + 6
    for flags in range(0, 32, 2):
        assert gzip.decompress(gzip_member(d.finish(), text, flags)) == text
    assert zlib_inflate(dw.gzip_stream([gzip_member(d.finish(), text, dw.FNAME), gzip_member(d.finish(), text, dw.FHCRC)])) == (text + text, 2)
    for kw in ({"crc": 1}, {"isize": 5}):
        with pytest.raises(zlib.error, match="incorrect"):
            zlib_inflate(gzip_member(d.finish(), text, **kw))


@pytest.mark.parametrize("name", VALID)
def test_valid_case_is_zlibs_text(name):
    blob, text = CASES[name]
    assert zlib_inflate(blob) == (text, MEMBERS[name])


@pytest.mark.parametrize("name", WRONG)
def test_wrong_case_is_refused_by_zlib(name):
    with pytest.raises(zlib.error, match=REFUSED[name]):
        zlib_inflate(CASES[name][0])


@pytest.mark.parametrize("name", sorted(DEVICE))
def test_device_case_fits_a_decoder(name):
    """under 16x overall, and no 4096 compressed bytes anywhere in the file give a decoder's arena of text or more"""
    blob, text = CASES[name]
    assert len(text) < 16 * len(blob)
    d = zlib.decompressobj(31)
    worst = 0
    for i in range(0, len(blob), CHUNK):
        piece, got = blob[i:i + CHUNK], 0
        while piece:
            got += len(d.decompress(piece))
            piece = d.unused_data if d.eof else b""
            if d.eof:                                   # the next member, or the zero padding after the last one
                d = zlib.decompressobj(31)
                piece = piece.lstrip(b"\0")
        worst = max(worst, got)
    assert worst <= CAP, worst


def test_the_cases_the_issue_names_are_there():
    for n in ("far_matches", "long_codes", "single_distance_code", "empty_distance_code", "eob_only_block", "hlit_hdist_max", "stored_65535",
              "flush_markers_sync", "flush_markers_full", "nested_gzip", "nested_gzip_4k_members", "chunk_start_twin_distance_50"):
        assert n in VALID
    assert sum(n.startswith("stored_align_pad") for n in VALID) == 8 and sum(n.startswith("zlib_wbits") for n in VALID) == 4
    assert len(WRONG) == 23 and LENIENT <= set(WRONG) and len(LENIENT) == 11


def test_wrong_cases_carry_a_real_trailer():
    """after the wrong block come a good last block and the trailer of real text: ISIZE counts the good blocks' literals at least"""
    for name in WRONG:
        blob = CASES[name][0]
        assert int.from_bytes(blob[-4:], "little") >= 150 and blob[-8:-4] != bytes(4), name
