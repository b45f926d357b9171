"""KmerTable: the HBM-resident canonical k-mer count table and the operations of the hot path on it.

Host-side mirror of what the reference does through `jellyfish count/histo` (src/jasper.sh:177,189) and the SWIG
module `dna_jellyfish` (JF::swig/mer_file.i, JF::swig/mer_dna.i).  All compute happens in libjasper_hip.so;
nothing here falls back to the CPU.
"""
import ctypes as C
import os

from . import _lib
from ._lib import FixRec, check


class PolishResult:
    """what one `jasper.py` process produces for one batch file (src/jasper.py:107-128).

    The polished texts stay in the C result object until asked for: `seq_view(i)` is a zero-copy memoryview,
    `seqs` materialises python objects (str if the inputs were str, else bytes) on first use."""

    def __init__(self, lib, handle, n_chunks, want_str, raw_records, aux, qv, lookups, seconds):
        self._L = lib
        self._h = handle
        self._n = n_chunks
        self._want_str = want_str
        self._seqs = None
        self._raw = raw_records     # numpy structured array (FixRec layout), ordered by chunk, pass, emission
        self._records = None
        self.aux = aux              # per chunk: bytes referenced by its 'x' records
        self.qv = qv                # (bad0, total0, badP, totalP)
        self.lookups = lookups
        self.seconds = seconds
        self.segments = 0
        self.respeculated = 0
        self.retried = False

    def __del__(self):
        try:
            if self._h:
                self._L.jasper_result_free(self._h)
                self._h = None
        except Exception:
            pass

    def seq_view(self, i):
        p = C.c_void_p()
        ln = C.c_int64(0)
        check(self._L.jasper_result_seq(self._h, i, C.byref(p), C.byref(ln)))
        if not ln.value:
            return memoryview(b"")
        return memoryview((C.c_char * ln.value).from_address(p.value)).cast("B")

    def seq_len(self, i):
        ln = C.c_int64(0)
        check(self._L.jasper_result_seq_len(self._h, i, C.byref(ln)))
        return ln.value

    def qv_chunk(self, i):
        """(bad0, total0, badP, totalP) of chunk record i alone"""
        q = (C.c_int64 * 4)()
        check(self._L.jasper_result_qv_chunk(self._h, i, q))
        return tuple(q)

    def seq_device(self, i):
        """(device pointer, length) of polished chunk i while the text is still in HBM (polish_batch_device results, until
        the next polish call on the same table or the first host access)"""
        p = C.c_void_p()
        ln = C.c_int64(0)
        check(self._L.jasper_result_seq_device(self._h, i, C.byref(p), C.byref(ln)))
        return (p.value or 0), ln.value

    @property
    def seqs(self):
        if self._seqs is None:
            out = []
            for i in range(self._n):
                raw = bytes(self.seq_view(i))
                out.append(raw.decode("latin-1") if self._want_str else raw)
            self._seqs = out
        return self._seqs

    @property
    def n_records(self):
        return len(self._raw)

    def record(self, i):
        """record i as a dict (chunk, pass_, seqno, kind, index, newc, oldc, rep[, patch, orig])"""
        e = self._raw[i]
        d = dict(chunk=int(e["chunk"]), pass_=int(e["pass_"]), seqno=int(e["seqno"]), kind=chr(int(e["kind"])), index=int(e["index"]),
                 newc=chr(int(e["newc"])), oldc=chr(int(e["oldc"])), rep=int(e["rep"]))
        if d["kind"] == "x":
            a = self.aux[d["chunk"]]
            o, n = int(e["aux_off"]), int(e["aux_len"])
            d["patch"] = a[o:o + n].decode("latin-1")
            d["orig"] = a[o + n:o + n + d["rep"]].decode("latin-1")
        return d

    @property
    def records(self):
        """list of dicts (see record()); decoded on first use"""
        if self._records is None:
            self._records = [self.record(i) for i in range(len(self._raw))]
        return self._records


KMERRUN_DTYPE = [("start", "<i8"), ("n_kmers", "<u8"), ("n_absent", "<u8"), ("seq", "<u4"), ("min_count", "<u4")]


class KmerReport:
    """dense k-mer report of a set of sequences (include/jasper_hip.h: jasper_kmer_report): `counts[i]` = (windows, valid,
    unreliable, absent) of sequence i, `runs` = numpy structured array (KMERRUN_DTYPE) of the maximal runs of unreliable
    k-mers ordered by (seq, start), `seconds` = device time of the kernels."""

    def __init__(self, counts, runs, seconds, retried):
        self.counts = counts
        self.runs = runs
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, KmerReport) and self.counts == other.counts and self.runs.tobytes() == other.runs.tobytes()

    def run_tuples(self):
        """[(seq, start, n_kmers, n_absent, min_count)]"""
        return [(int(r["seq"]), int(r["start"]), int(r["n_kmers"]), int(r["n_absent"]), int(r["min_count"])) for r in self.runs]


class KmerSpectrum:
    """copy-number k-mer spectrum of a read table and an assembly table (include/jasper_hip.h: jasper_table_spectrum): `cells` =
    numpy uint64 array (6, 10002), cells[m][c] = distinct k-mers with min(copies in the assembly, 5) = m and min(count in the
    reads, 10001) = c (column 0: only in the assembly), `seconds` = device time of the two sweeps.  The numbers derived from it
    and the files: jasper_amd/spectra.py."""

    def __init__(self, cells, seconds):
        self.cells = cells
        self.seconds = seconds

    def __eq__(self, other):
        return isinstance(other, KmerSpectrum) and self.cells.shape == other.cells.shape and bool((self.cells == other.cells).all())


COPYRUN_DTYPE = [("start", "<i8"), ("n_kmers", "<u8"), ("sum_reads", "<u8"), ("sum_asm", "<u8"), ("seq", "<u4"), ("kind", "<u4")]
COPY_KINDS = {1: "excess", 2: "deficit"}


class CopyReport:
    """copy-number scan of a set of sequences against the reads' table and the assembly's (include/jasper_hip.h:
    jasper_copy_report): `counts[i]` = (windows, valid, excess, deficit, sum_reads, sum_asm) of sequence i, `runs` = numpy
    structured array (COPYRUN_DTYPE) of the maximal runs of one class (kind 1 = excess, 2 = deficit) ordered by (seq, start),
    `seconds` = device time of the kernels.  The files made from it: jasper_amd/copies.py."""

    def __init__(self, counts, runs, seconds, retried):
        self.counts = counts
        self.runs = runs
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, CopyReport) and self.counts == other.counts and self.runs.tobytes() == other.runs.tobytes()

    def run_tuples(self):
        """[(seq, start, n_kmers, kind, sum_reads, sum_asm)]"""
        return [(int(r["seq"]), int(r["start"]), int(r["n_kmers"]), int(r["kind"]), int(r["sum_reads"]), int(r["sum_asm"])) for r in self.runs]


class PairSpectrum:
    """pair spectrum of a read table and the tables of both haplotypes of a diploid assembly (include/jasper_hip.h:
    jasper_table_spectrum_pair): `cells` = numpy uint64 array (4, 10002), cells[j][c] = distinct k-mers with j = (in asm ? 1 : 0) |
    (in alt ? 2 : 0) and min(count in the reads, 10001) = c (column 0: not in the reads), `seconds` = device time of the three
    sweeps.  The numbers derived from it and the files: jasper_amd/diploid.py."""

    def __init__(self, cells, seconds):
        self.cells = cells
        self.seconds = seconds

    def __eq__(self, other):
        return isinstance(other, PairSpectrum) and self.cells.shape == other.cells.shape and bool((self.cells == other.cells).all())


PAIRRUN_DTYPE = [("start", "<i8"), ("n_kmers", "<u8"), ("sum_reads", "<u8"), ("seq", "<u4"), ("kind", "<u4")]
PAIR_KINDS = {1: "solid", 2: "weak"}


class PairScan:
    """scan of one haplotype's sequences against the reads' table and the other haplotype's (include/jasper_hip.h:
    jasper_pair_scan): `counts[i]` = (windows, valid, unreliable, absent, private_solid, private_weak) of sequence i, `runs` = numpy
    structured array (PAIRRUN_DTYPE) of the maximal runs of one class (kind 1 = private and solid, 2 = private and weak) ordered
    by (seq, start), `seconds` = device time of the kernels.  The files made from it: jasper_amd/diploid.py."""

    def __init__(self, counts, runs, seconds, retried):
        self.counts = counts
        self.runs = runs
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, PairScan) and self.counts == other.counts and self.runs.tobytes() == other.runs.tobytes()

    def run_tuples(self):
        """[(seq, start, n_kmers, kind, sum_reads)]"""
        return [(int(r["seq"]), int(r["start"]), int(r["n_kmers"]), int(r["kind"]), int(r["sum_reads"])) for r in self.runs]


DUPRUN_DTYPE = [("start", "<i8"), ("mate_start", "<i8"), ("n_kmers", "<u8"), ("sum_reads", "<u8"), ("n_deficit", "<u8"), ("seq", "<u4"), ("mate_seq", "<u4"),
                ("strand", "<u4"), ("pad", "<u4")]


class DupMap:
    """duplication map of a set of sequences against the reads' table and the assembly's (include/jasper_hip.h: jasper_dup_map):
    `counts[i]` = (windows, valid, two_copy, deficit, multi, unplaced, sum_reads) of sequence i, `runs` = numpy structured array
    (DUPRUN_DTYPE) of the maximal colinear runs of two-copy windows ordered by (seq, start), each with the sequence and the leftmost
    window of its mate stretch and the strand (0 = `+`, 1 = `-`), `seconds` = (device time of the index pass, of the scan).  The
    files made from it: jasper_amd/dups.py."""

    def __init__(self, counts, runs, seconds, retried):
        self.counts = counts
        self.runs = runs
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, DupMap) and self.counts == other.counts and self.runs.tobytes() == other.runs.tobytes()

    def run_tuples(self):
        """[(seq, start, n_kmers, mate_seq, mate_start, strand, sum_reads, n_deficit)]"""
        return [(int(r["seq"]), int(r["start"]), int(r["n_kmers"]), int(r["mate_seq"]), int(r["mate_start"]), int(r["strand"]), int(r["sum_reads"]),
                 int(r["n_deficit"])) for r in self.runs]


HAPRUN_DTYPE = [("start", "<i8"), ("n_kmers", "<u8"), ("seq", "<u4"), ("kind", "<u4")]
HAP_KINDS = {1: "mat", 2: "pat"}


class HapmerScan:
    """trio hap-mer scan of a set of sequences against the mother's, the father's and (optionally) the child's table
    (include/jasper_hip.h: jasper_hapmer_scan): `counts[i]` = (windows, valid, mat, pat) of sequence i, `runs` = numpy structured
    array (HAPRUN_DTYPE) of the maximal runs of one class = the markers (kind 1 = mat, 2 = pat) ordered by (seq, start), `seconds`
    = device time of the kernels.  The phase blocks and the files made from it: jasper_amd/hapmers.py."""

    def __init__(self, counts, runs, seconds, retried):
        self.counts = counts
        self.runs = runs
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, HapmerScan) and self.counts == other.counts and self.runs.tobytes() == other.runs.tobytes()

    def run_tuples(self):
        """[(seq, start, n_kmers, kind)]"""
        return [(int(r["seq"]), int(r["start"]), int(r["n_kmers"]), int(r["kind"])) for r in self.runs]


class HapmerCensus:
    """hap-mer census of a trio's tables against an assembly's (include/jasper_hip.h: jasper_hapmer_census): `mat` and `pat` =
    (hapmers, found, occurrences), `seconds` = device time of the two sweeps"""

    def __init__(self, mat, pat, seconds):
        self.mat = mat
        self.pat = pat
        self.seconds = seconds

    def __eq__(self, other):
        return isinstance(other, HapmerCensus) and self.mat == other.mat and self.pat == other.pat


class ReadBins:
    """trio read binning of a batch of reads (include/jasper_hip.h: jasper_read_bins): `mat[i]` / `pat[i]` = the windows of read i whose
    k-mer only the mother's / only the father's reads hold (np.uint32[n]), `seconds` = device time of the kernels.  The rule that makes
    bins of them and the files: jasper_amd/triobin.py."""

    def __init__(self, mat, pat, seconds):
        self.mat = mat
        self.pat = pat
        self.seconds = seconds

    def __eq__(self, other):
        return isinstance(other, ReadBins) and self.mat.tobytes() == other.mat.tobytes() and self.pat.tobytes() == other.pat.tobytes()


READ_TEXT_FORMATS = {"fastq": 0, "fasta": 1}


class ReadText:
    """one chunk of raw FASTQ / FASTA text parsed, packed and binned on the GPU (include/jasper_hip.h: jasper_read_text_bins): `used` =
    the bytes whole records cover, `n_records`; `malformed` with `bad_record`, and then nothing else; otherwise `rec_start`
    (np.int64[n + 1], the last = used), `head_end`, `lens` (np.int64[n]), `mat` / `pat` (np.uint32[n]) as ReadBins has them, `seq` (the
    packed sequences, np.uint8, when asked for), `seconds` = device time of the binning kernels, `index_seconds` = of index + pack."""

    def __init__(self, used, n_records, malformed, bad_record, seconds, index_seconds):
        self.used, self.n_records, self.malformed, self.bad_record = used, n_records, malformed, bad_record
        self.seconds, self.index_seconds = seconds, index_seconds
        self.rec_start = self.head_end = self.lens = self.mat = self.pat = self.seq = None
        self.no_format, self.inflate_seconds = False, 0.0      # (a gz session's: GzText.bins)


GZ_TEXT_FORMATS = {None: 0, "fastq": 1, "fasta": 2}
GZ_STATS = ("decoders", "accepted", "device_bytes", "host_bytes", "slabs", "members")


class RoutedText:
    """a block of text routed on the GPU (include/jasper_hip.h: jasper_route_text): `out` = three np.uint8 arrays, the bytes of bin 0, 1
    and 2 in input order (views of the buffers handed in, or of fresh ones), `mismatches` = segments that do not begin with the expected
    byte, `seconds` = device time of the kernels; from a gz session `got` = inflated bytes pulled (nothing is routed when that is not
    bounds[-1]: `routed` False) and `inflate_seconds`.  With gz=True `out` holds each bin's bytes as BGZF members (jasper_route_text_gz),
    `raw_bytes` = the routed bytes per bin, `deflate` = the compressor's counters (DEFLATE_COUNTERS), `deflate_seconds` its kernels' time."""

    def __init__(self, out, mismatches, seconds, got=None, routed=True, inflate_seconds=0.0, raw_bytes=None, deflate=None, deflate_seconds=0.0):
        self.out, self.mismatches, self.seconds, self.got, self.routed, self.inflate_seconds = out, mismatches, seconds, got, routed, inflate_seconds
        self.raw_bytes, self.deflate, self.deflate_seconds = raw_bytes, deflate, deflate_seconds


DEFLATE_COUNTERS = ("blocks", "stored", "literal_only", "lz", "matches", "matched_bytes")


def deflate_bound(n):
    """bytes that the BGZF members of n text bytes come to at the most (jasper_deflate_bound)"""
    return int(_lib.lib().jasper_deflate_bound(int(n)))


def _route_call(L, th, session, buf, n, room, bounds, bins, first, check_from, out, gz):
    """what KmerTable.route_text (session None: buf = the text, n its length) and GzText.route (buf None, n = want) share: the arguments
    made ready, the one of the four C calls that matches -- a session's or not, BGZF members or not -- and its RoutedText"""
    import numpy as np
    if gz:
        room = deflate_bound(room)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64)
    bins = np.ascontiguousarray(bins, dtype=np.uint8)
    if bounds.ndim != 1 or bins.ndim != 1 or len(bounds) != len(bins) + 1:
        raise ValueError("route: bounds must hold one value more than bins")
    if isinstance(first, (bytes, str)):
        first = ord(first) if len(first) else 0         # (an empty file has no records and no first byte: nothing is compared)
    if out is None:
        out = [np.empty(max(room, 1), dtype=np.uint8) for _ in range(3)]
    if len(out) != 3 or any(o.dtype != np.uint8 or o.ndim != 1 or not o.flags.c_contiguous or len(o) < room for o in out):
        raise ValueError("route: out must be three contiguous np.uint8 arrays with room for the text")
    vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    nb, raw, cnt, got, bad, secs = (C.c_int64 * 3)(), (C.c_int64 * 3)(), (C.c_uint64 * 6)(), C.c_int64(0), C.c_int64(0), (C.c_double * 3)()
    src = (th, vp(buf) if buf.size else None, n) if session is None else (session._handle(), th, n)
    job = (len(bins), vp(bounds), vp(bins) if len(bins) else None, int(first), int(check_from), vp(out[0]), vp(out[1]), vp(out[2]))
    outs = ((C.c_int64 * 3)(*(len(o) for o in out)), nb, raw) if gz else (nb,)
    rest = (() if session is None else (C.byref(got),)) + (C.byref(bad),) + ((cnt,) if gz else ()) + (secs,)
    check(getattr(L, ("jasper_route_text" if session is None else "jasper_gz_text_route") + ("_gz" if gz else ""))(*src, *job, *outs, *rest))
    # device_seconds: the kernels, then a session's pull, then the compressor (include/jasper_hip.h)
    pull, deflate = (0.0, secs[1]) if session is None else (secs[1], secs[2])
    routed = session is None or got.value == int(bounds[-1])
    r = RoutedText([o[:nb[b]] for b, o in enumerate(out)] if routed else None, bad.value, secs[0], None if session is None else got.value, routed, pull)
    if gz:
        r.raw_bytes, r.deflate, r.deflate_seconds = [int(v) for v in raw], dict(zip(DEFLATE_COUNTERS, (int(v) for v in cnt))), deflate
    return r


def _fetch_records(L, mh, r, want_seq=False):
    """the per-record arrays of the clean ReadText r, from the maternal table's workspace (jasper_read_text_fetch) -> r"""
    import numpy as np
    nr = r.n_records
    r.rec_start, r.head_end, r.lens = np.zeros(nr + 1, dtype=np.int64), np.zeros(nr, dtype=np.int64), np.zeros(nr, dtype=np.int64)
    r.mat, r.pat = np.zeros(nr, dtype=np.uint32), np.zeros(nr, dtype=np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    check(L.jasper_read_text_fetch(mh, nr, vp(r.rec_start), vp(r.head_end), vp(r.lens), vp(r.mat), vp(r.pat), None))
    if want_seq:                                    # (its size is the sum of lens: a second fetch, for tests)
        r.seq = np.zeros(int(r.lens.sum()), dtype=np.uint8)
        check(L.jasper_read_text_fetch(mh, nr, vp(r.rec_start), vp(r.head_end), vp(r.lens), vp(r.mat), vp(r.pat), vp(r.seq) if r.seq.size else None))
    return r


class GzText:
    """a .gz read file inflated on the GPU, its text handed to the read-text path inside HBM (include/jasper_hip.h: jasper_gz_text_open).
    Made by KmerTable.gz_text(path); a context manager.  `n` = bytes of the current call's text, `eof` = the inflater has ended."""

    def __init__(self, table, path):
        self._t, self._L, self.path = table, table._L, path
        h = C.c_void_p()
        check(self._L.jasper_gz_text_open(table._h, os.fsencode(path), C.byref(h)))
        self._g = h
        self.n, self.eof, self.fmt, self.inflate_seconds = 0, False, None, 0.0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._g is not None:
            self._L.jasper_gz_text_close(self._g)
            self._g = None

    def _handle(self):
        if self._g is None:
            raise ValueError("gz_text: the session is closed")
        return self._g

    def bins(self, pat, want, fmt, thre_mat, thre_pat):
        """one chunk: the tail the call before left unused, then up to `want` more inflated bytes -> ReadText (no_format: the first byte
        is neither @ nor >).  fmt: None on the first call (the first byte decides; self.fmt says what), then "fastq" / "fasta" """
        if fmt not in GZ_TEXT_FORMATS:
            raise ValueError("gz_text: fmt must be None, 'fastq' or 'fasta'")
        ph = KmerTable._parent_handle(pat, "paternal", "gz_text")
        used, nrec, bad, n = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        status, eof, f, secs = C.c_int(0), C.c_int(0), C.c_int(GZ_TEXT_FORMATS[fmt]), (C.c_double * 3)()
        check(self._L.jasper_gz_text_bins(self._handle(), self._t._h, ph, int(want), C.byref(f), _thre32(thre_mat), _thre32(thre_pat), C.byref(n), C.byref(eof), C.byref(used),
                                          C.byref(nrec), C.byref(status), C.byref(bad), secs))
        self.n, self.eof, self.fmt = n.value, bool(eof.value), {0: None, 1: "fastq", 2: "fasta"}[f.value]
        self.inflate_seconds += secs[2]
        r = ReadText(used.value, nrec.value, status.value == 1, bad.value, secs[1], secs[0])
        r.no_format, r.inflate_seconds = status.value == 2, secs[2]
        if r.malformed or r.no_format:
            return r
        return _fetch_records(self._L, self._t._h, r)

    def text(self, start, length):
        """bytes [start, start + length) of the current call's text -> np.uint8"""
        import numpy as np
        out = np.empty(int(length), dtype=np.uint8)
        check(self._L.jasper_gz_text_copy(self._handle(), int(start), int(length), C.c_void_p(out.ctypes.data) if out.size else None))
        return out

    def stats(self):
        """decoders, accepted, device_bytes, host_bytes, slabs, members: as KmerTable.last_inflate"""
        st = (C.c_uint64 * 6)()
        check(self._L.jasper_gz_text_stats(self._handle(), st))
        return dict(zip(GZ_STATS, (int(v) for v in st)))

    def route(self, want, bounds, bins, first, check_from=0, out=None, gz=False):
        """the next `want` inflated bytes routed as KmerTable.route_text routes a host text -> RoutedText with `got`"""
        r = _route_call(self._L, self._t._h, self, None, int(want), int(bounds[-1]) if len(bounds) else 0, bounds, bins, first, check_from, out, gz)
        self.inflate_seconds += r.inflate_seconds
        return r


VARIANT_DTYPE = [("pos", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("alt_min", "<u4"), ("ref", "u1"), ("alt", "u1"), ("kind", "u1"), ("pad", "u1")]
VARIANT_KINDS = {1: "het", 2: "error"}


class VariantScan:
    """variant scan of a set of sequences against the reads' table (include/jasper_hip.h: jasper_variant_scan): `counts[i]` =
    (evaluated, het, error) of sequence i, `records` = numpy structured array (VARIANT_DTYPE) of the substitution sites (kind 1 =
    het, 2 = error; ref / alt are the letters' byte values) ordered by (seq, pos, alt), `candidates` = what the dense scan handed
    to the check, `seconds` = device time of the kernels.  The files made from it: jasper_amd/variants.py."""

    def __init__(self, counts, records, candidates, seconds, retried):
        self.counts = counts
        self.records = records
        self.candidates = candidates
        self.seconds = seconds
        self.retried = retried

    def __eq__(self, other):
        return (isinstance(other, VariantScan) and self.counts == other.counts and self.candidates == other.candidates
                and self.records.tobytes() == other.records.tobytes())

    def record_tuples(self):
        """[(seq, pos, ref, alt, ref_min, alt_min, kind)], ref and alt as one-letter strings"""
        return [(int(r["seq"]), int(r["pos"]), chr(int(r["ref"])), chr(int(r["alt"])), int(r["ref_min"]), int(r["alt_min"]), int(r["kind"])) for r in self.records]


INDEL_DTYPE = [("pos", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("alt_min", "<u4"), ("len", "<u2"), ("type", "u1"), ("base", "u1"), ("kind", "u1"),
               ("pad", "u1", (7,))]
INDEL_TYPES = {1: "ins", 2: "del"}


MIXED_DTYPE = [("pos", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("alt_min", "<u4"), ("bases", "<u4"), ("len", "<u2"), ("kind", "u1"), ("pad", "u1", (5,))]


class MixedInsertions:
    """the mixed half of an indel scan (include/jasper_hip.h: jasper_indel_scan_mixed): `counts[i]` = (mixed_het, mixed_error, complex)
    of sequence i, `records` = numpy structured array (MIXED_DTYPE) of the insertions of mixed bases ordered by (seq, pos, len, inserted
    string; base i of it is bits 2i..2i+1 of `bases`, A C G T = 0 1 2 3), `seconds` = device time of the search kernel, `lookups` =
    table lookups it made, `retried` = it was repeated with a larger record list."""

    def __init__(self, counts, records, seconds, lookups, retried):
        self.counts = counts
        self.records = records
        self.seconds = seconds
        self.lookups = lookups
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, MixedInsertions) and self.counts == other.counts and self.records.tobytes() == other.records.tobytes()

    def record_tuples(self):
        """[(seq, pos, len, y, ref_min, alt_min, kind)], y = the inserted string"""
        return [(int(r["seq"]), int(r["pos"]), int(r["len"]), "".join("ACGT"[(int(r["bases"]) >> (2 * i)) & 3] for i in range(int(r["len"]))),
                 int(r["ref_min"]), int(r["alt_min"]), int(r["kind"])) for r in self.records]


class IndelScan:
    """indel scan of a set of sequences against the reads' table (include/jasper_hip.h: jasper_indel_scan): `counts[i]` = (ins_het,
    ins_error, del_het, del_error) of sequence i, `records` = numpy structured array (INDEL_DTYPE) of the insertions (type 1) and
    deletions (type 2) ordered by (seq, pos, type, len, base), `variants` = the VariantScan of the same input (one dense scan serves
    both), `seconds` = device time of the scan and all check kernels, `check_seconds` = of the indel check alone, `lookups` = table
    lookups that check made, `mixed` = None or the MixedInsertions of a scan with mixed=True (not part of ==: a scan with it equals
    the scan without it), `clusters` = None or the HetClusters of a scan with clusters=N (not part of == either).  The files made from
    it: jasper_amd/indels.py, jasper_amd/hetclusters.py."""

    def __init__(self, counts, records, variants, seconds, check_seconds, lookups, retried, mixed=None, clusters=None):
        self.counts = counts
        self.records = records
        self.variants = variants
        self.seconds = seconds
        self.check_seconds = check_seconds
        self.lookups = lookups
        self.retried = retried
        self.mixed = mixed
        self.clusters = clusters

    def __eq__(self, other):
        return (isinstance(other, IndelScan) and self.counts == other.counts and self.records.tobytes() == other.records.tobytes()
                and self.variants == other.variants)

    def record_tuples(self):
        """[(seq, pos, 'ins' | 'del', len, base, ref_min, alt_min, kind)], base as a one-letter string"""
        return [(int(r["seq"]), int(r["pos"]), INDEL_TYPES[int(r["type"])], int(r["len"]), chr(int(r["base"])), int(r["ref_min"]), int(r["alt_min"]),
                 int(r["kind"])) for r in self.records]


COMPOUND_DTYPE = [("pos", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("alt_min", "<u4"), ("ref_len", "<u4"), ("bases", "<u8", (2,)), ("len", "<u2"),
                  ("pad", "u1", (6,))]


def compound_string(bases, length):
    """y of a compound record: base i is bits 2i..2i+1 of bases[i // 32], A C G T = 0 1 2 3"""
    return "".join("ACGT"[(int(bases[i >> 5]) >> (2 * (i & 31))) & 3] for i in range(int(length)))


class CompoundScan:
    """compound scan of a set of sequences against the reads' table (include/jasper_hip.h: jasper_compound_scan): `counts[i]` = (sites,
    bridged, records, long, complex) of sequence i, `records` = numpy structured array (COMPOUND_DTYPE) of the replacements the reads
    hold for clusters of differences, ordered by (seq, pos, len, y), `report` = the KmerReport of the same input (one dense scan
    serves both), `seconds` = device time of the dense scan and the search, `search_seconds` = of the search kernel alone, `lookups`
    = table lookups it made, `retried` = it was repeated with a larger record list.  The files made from it: jasper_amd/compound.py."""

    def __init__(self, counts, records, report, seconds, search_seconds, lookups, retried):
        self.counts = counts
        self.records = records
        self.report = report
        self.seconds = seconds
        self.search_seconds = search_seconds
        self.lookups = lookups
        self.retried = retried

    def __eq__(self, other):
        return (isinstance(other, CompoundScan) and self.counts == other.counts and self.records.tobytes() == other.records.tobytes()
                and self.report == other.report)

    def record_tuples(self):
        """[(seq, pos, ref_len, len, y, ref_min, alt_min)], y = the replacement"""
        return [(int(r["seq"]), int(r["pos"]), int(r["ref_len"]), int(r["len"]), compound_string(r["bases"], r["len"]), int(r["ref_min"]), int(r["alt_min"]))
                for r in self.records]


HET_CLUSTER_DTYPE = COMPOUND_DTYPE


class HetClusters:
    """the het-cluster half of an indel scan (include/jasper_hip.h: jasper_indel_scan_clusters): `counts[i]` = (searched, sites, records,
    complex) of sequence i, `records` = numpy structured array (HET_CLUSTER_DTYPE, the layout of COMPOUND_DTYPE) of the replacements
    where the sequence and the reads' other haplotype are both solid, ordered by (seq, pos, ref_len, len, y), `seconds` = device time
    of the search kernel, `lookups` = table lookups it made, `retried` = it was repeated with a larger record list.  The files made
    from it: jasper_amd/hetclusters.py."""

    def __init__(self, counts, records, seconds, lookups, retried):
        self.counts = counts
        self.records = records
        self.seconds = seconds
        self.lookups = lookups
        self.retried = retried

    def __eq__(self, other):
        return isinstance(other, HetClusters) and self.counts == other.counts and self.records.tobytes() == other.records.tobytes()

    def record_tuples(self):
        """[(seq, pos, ref_len, len, y, ref_min, alt_min)], y = the replacement"""
        return [(int(r["seq"]), int(r["pos"]), int(r["ref_len"]), int(r["len"]), compound_string(r["bases"], r["len"]), int(r["ref_min"]), int(r["alt_min"]))
                for r in self.records]


GAP_SITE_DTYPE = [("a", "<i8"), ("q", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("n_records", "<u4"), ("levels", "<u4"), ("trim_left", "<u4"), ("trim_right", "<u4"),
                  ("kind", "u1"), ("status", "u1"), ("pad", "u1", (6,))]
GAP_FILL_DTYPE = [("pos", "<i8"), ("bases_off", "<u8"), ("seq", "<u4"), ("ref_len", "<u4"), ("len", "<u4"), ("alt_min", "<u4")]
GAP_KINDS = {0: "explicit", 1: "gap", 2: "run"}
GAP_STATUS = {1: "dead", 2: "limit", 3: "complex", 4: "edge", 5: "ragged", 6: "skipped"}


def make_gap_sites(sites):
    """[(seq, a, q)] or [(seq, a, q, ref_min)] -> structured array (GAP_SITE_DTYPE) as KmerTable.gap_search takes it"""
    import numpy as np
    arr = np.zeros(len(sites), dtype=GAP_SITE_DTYPE)
    for i, s in enumerate(sites):
        arr[i]["seq"], arr[i]["a"], arr[i]["q"] = s[0], s[1], s[2]
        arr[i]["ref_min"] = s[3] if len(s) > 3 else 0
    return arr


class GapScan:
    """gap scan of a set of sequences against the reads' table (include/jasper_hip.h: jasper_gap_scan): `counts[i]` = (sites, searched,
    bridged, unique, records, edge, ragged, limit, complex) of sequence i, `sites` = numpy structured array (GAP_SITE_DTYPE) ordered by
    (seq, a), `records` = numpy structured array (GAP_FILL_DTYPE) of the fills the reads hold, ordered by (seq, pos, len, y), whose
    bases are `bases[bases_off : bases_off + len]`, `report` = the KmerReport of the same input (None after gap_search), `seconds` =
    device time of the dense scans and the search, `search_seconds` = of the search kernel alone, `runs_seconds` = of the
    invalid-window scan, `lookups` = table lookups the search made, `retried` = it was repeated with larger lists.  The files made
    from it: jasper_amd/gaps.py."""

    def __init__(self, counts, sites, records, bases, report, seconds, search_seconds, runs_seconds, lookups, retried):
        self.counts = counts
        self.sites = sites
        self.records = records
        self.bases = bases
        self.report = report
        self.seconds = seconds
        self.search_seconds = search_seconds
        self.runs_seconds = runs_seconds
        self.lookups = lookups
        self.retried = retried

    def __eq__(self, other):
        return (isinstance(other, GapScan) and self.counts == other.counts and self.sites.tobytes() == other.sites.tobytes()
                and self.records.tobytes() == other.records.tobytes() and self.bases == other.bases and self.report == other.report)

    def fill(self, r):
        """y of a record"""
        return self.bases[int(r["bases_off"]):int(r["bases_off"]) + int(r["len"])].decode("latin-1")

    def record_tuples(self):
        """[(seq, pos, ref_len, len, y, ref_min, alt_min)], y = the fill, ref_min = its site's"""
        rmin = {(int(s["seq"]), int(s["a"])): int(s["ref_min"]) for s in self.sites}
        return [(int(r["seq"]), int(r["pos"]), int(r["ref_len"]), int(r["len"]), self.fill(r), rmin[(int(r["seq"]), int(r["pos"]))], int(r["alt_min"]))
                for r in self.records]

    def site_tuples(self):
        """[(seq, a, q, kind, status, n_records, levels, trim_left, trim_right, ref_min)], kind = 'gap' | 'run' | 'explicit', status = 'dead' |
        'limit' | 'complex' | 'edge' | 'ragged' | 'skipped'"""
        return [(int(s["seq"]), int(s["a"]), int(s["q"]), GAP_KINDS[int(s["kind"])], GAP_STATUS[int(s["status"])], int(s["n_records"]), int(s["levels"]),
                 int(s["trim_left"]), int(s["trim_right"]), int(s["ref_min"])) for s in self.sites]


EDIT_DTYPE = [("pos", "<i8"), ("seq", "<u4"), ("ref_min", "<u4"), ("alt_min", "<u4"), ("ref_len", "<u4"), ("bases", "<u8", (2,)), ("len", "<u2"), ("source", "u1"),
              ("round", "u1"), ("pad", "u1", (4,))]
EDIT_SOURCES = {1: "sub", 2: "ins", 3: "del", 4: "mixed", 5: "compound"}


def make_edits(edits):
    """[(seq, pos, ref_len, y)] -> structured array (EDIT_DTYPE) as KmerTable.apply_edits takes it; y a str or bytes of ACGT"""
    import numpy as np
    arr = np.zeros(len(edits), dtype=EDIT_DTYPE)
    for i, (seq, pos, rlen, y) in enumerate(edits):
        y = y if isinstance(y, str) else bytes(y).decode("latin-1")
        v = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(y))
        arr[i] = (pos, seq, 0, 0, rlen, [v & (2**64 - 1), v >> 64], len(y), 0, 0, [0] * 4)
    return arr


class Repair:
    """the repair stage on a set of sequences (include/jasper_hip.h: jasper_repair): `seqs` = the final sequences as bytes, `edits` =
    numpy structured array (EDIT_DTYPE) of every applied edit ordered by (round, seq, pos), pos in the coordinates of that round's
    input, `rounds` = [(records, accepted, conflicts, ambiguous, unreliable_before, unreliable_after)] of every round that scanned,
    `before` / `after` = the KmerReport of the input and of the final sequences, `seconds` = device time of the scans and the apply
    kernel, `apply_seconds` = of the apply kernel alone.  The files made from it: jasper_amd/repair.py."""

    def __init__(self, seqs, edits, rounds, before, after, seconds, apply_seconds):
        self.seqs = seqs
        self.edits = edits
        self.rounds = rounds
        self.before = before
        self.after = after
        self.seconds = seconds
        self.apply_seconds = apply_seconds

    def __eq__(self, other):
        return (isinstance(other, Repair) and self.seqs == other.seqs and self.edits.tobytes() == other.edits.tobytes() and self.rounds == other.rounds
                and self.before == other.before and self.after == other.after)

    def edit_tuples(self):
        """[(round, seq, pos, ref_len, y, source, ref_min, alt_min)], y = the replacement, source = 'sub' | 'ins' | 'del' | 'mixed' | 'compound'"""
        return [(int(e["round"]), int(e["seq"]), int(e["pos"]), int(e["ref_len"]), compound_string(e["bases"], e["len"]), EDIT_SOURCES[int(e["source"])],
                 int(e["ref_min"]), int(e["alt_min"])) for e in self.edits]


FIXREC_DTYPE = [("index", "<i8"), ("chunk", "<u4"), ("seqno", "<u4"), ("pass_", "u1"), ("kind", "u1"), ("newc", "u1"), ("oldc", "u1"),
                ("rep", "<u4"), ("aux_off", "<u4"), ("aux_len", "<u4")]


def _peak32(peak):
    """peak as the C-ABI's uint32 (a value outside its range is an error here, not a silent wrap)"""
    p = int(peak)
    if p < 0 or p > 0xFFFFFFFF:
        raise ValueError("peak must be in [1, 2^32-1]")
    return p


def _thre32(thre):
    """a threshold as the C-ABI's uint32 (0 passes: the library refuses it with a message that names it)"""
    t = int(thre)
    if t < 0 or t > 0xFFFFFFFF:
        raise ValueError("a threshold must be in [1, 2^32-1]")
    return t


def _seq_args(seqs):
    """sequences (str or bytes) as the arguments of a host-text entry point: (n, char *[n], int64 lens[n])"""
    n = len(seqs)
    bs = [s.encode("latin-1") if isinstance(s, str) else (s if isinstance(s, bytes) else bytes(s)) for s in seqs]
    return n, (C.c_char_p * max(n, 1))(*bs), (C.c_int64 * max(n, 1))(*[len(b) for b in bs])


def _text_args(d_text, offsets):
    """sequences back to back in HBM as the arguments of a device-text entry point: (n, void *, int64 offsets[n + 1]); d_text is a
    device pointer (int) or an object with .data_ptr()"""
    n = len(offsets) - 1
    ptr = d_text.data_ptr() if hasattr(d_text, "data_ptr") else int(d_text)
    return n, C.c_void_p(ptr), (C.c_int64 * (n + 1))(*[int(o) for o in offsets])


def _counts(num_seqs_fn, counts_fn, res, width):
    """the `width` counters per sequence of a scan's result -> list of tuples"""
    out = []
    c = (C.c_uint64 * width)()
    for i in range(num_seqs_fn(res)):
        check(counts_fn(res, i, c))
        out.append(tuple(int(v) for v in c))
    return out


def _records(records_fn, res, ctype, dtype):
    """the record array of a scan's result -> numpy structured array (a copy: the result may be freed)"""
    import numpy as np
    rp = C.POINTER(ctype)()
    rn = C.c_uint64(0)
    check(records_fn(res, C.byref(rp), C.byref(rn)))
    if rn.value:
        return np.frombuffer(C.string_at(rp, rn.value * C.sizeof(ctype)), dtype=dtype).copy()
    return np.zeros(0, dtype=dtype)


class KmerTable:
    def __init__(self, k, min_slots=1 << 20, device=0):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.k = int(k)
        self.device = int(device)
        check(self._L.jasper_table_create(self.k, int(min_slots), self.device, C.byref(self._h)))

    @classmethod
    def from_jf(cls, path, device=0):
        """jf.QueryMerFile(path): open a Jellyfish binary/sorted DB into HBM; k comes from the file (JF::swig/mer_file.i:18-36)"""
        self = cls.__new__(cls)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.device = int(device)
        check(self._L.jasper_table_load_jf(path.encode(), self.device, C.byref(self._h)))
        self.k = self.info()["k"]
        return self

    @classmethod
    def from_jf_part(cls, path, part, nparts, device=0):
        """records [n*part/nparts, n*(part+1)/nparts) of a Jellyfish DB: one GPU's shard of it"""
        self = cls.__new__(cls)
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.device = int(device)
        check(self._L.jasper_table_load_jf_part(path.encode(), self.device, int(part), int(nparts), C.byref(self._h)))
        self.k = self.info()["k"]
        return self

    def write_jf(self, path, cmdline=()):
        """write the table as a Jellyfish binary/sorted DB (what `jellyfish count -o` produces, src/jasper.sh:177)"""
        args = [a.encode() for a in cmdline]
        arr = (C.c_char_p * max(len(args), 1))(*args)
        check(self._L.jasper_table_write_jf(self._h, path.encode(), arr, len(args)))

    def write_jf_piece(self, path, cmdline, size_log2, what):
        """what: 0 = whole file, 1 = sorted records only (one GPU's piece), 2 = header only; `size` of the file = 2^size_log2"""
        args = [a.encode() for a in cmdline]
        arr = (C.c_char_p * max(len(args), 1))(*args)
        check(self._L.jasper_table_write_jf_piece(self._h, path.encode(), arr, len(args), int(size_log2), int(what)))

    def export_file_ranges(self, dev_ptr, cap_entries, n_ranges, size_log2):
        """entries grouped by their range in the order of a binary/sorted file of size 2^size_log2 (layout as export_owner)"""
        counts = (C.c_uint64 * int(n_ranges))()
        check(self._L.jasper_table_export_file_ranges(self._h, C.c_void_p(dev_ptr), int(cap_entries), int(n_ranges), int(size_log2), counts))
        return [int(c) for c in counts]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.jasper_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- counting (jellyfish count -C) -------------------------------------------------------------
    def count_files(self, paths):
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        check(self._L.jasper_count_reads_files(self._h, arr, len(paths)))

    def count_file_ranges(self, ranges):
        """ranges: list of (path, begin, end) byte ranges (end < 0: to the end of the file) -- one GPU's shard of the reads"""
        n = len(ranges)
        arr = (C.c_char_p * max(n, 1))(*[r[0].encode() for r in ranges])
        b = (C.c_int64 * max(n, 1))(*[int(r[1]) for r in ranges])
        e = (C.c_int64 * max(n, 1))(*[int(r[2]) for r in ranges])
        check(self._L.jasper_count_reads_file_ranges(self._h, arr, b, e, n))

    # ---- the read files as a feed of base batches in HBM (include/jasper_hip.h, jasper_read_feed_*) ----
    def feed_start(self, ranges):
        """ranges as for count_file_ranges; this table only lends its device and buffers"""
        n = len(ranges)
        arr = (C.c_char_p * max(n, 1))(*[r[0].encode() for r in ranges])
        b = (C.c_int64 * max(n, 1))(*[int(r[1]) for r in ranges])
        e = (C.c_int64 * max(n, 1))(*[int(r[2]) for r in ranges])
        check(self._L.jasper_read_feed_start(self._h, arr, b, e, n))

    def feed_next(self):
        """(device pointer, bytes) of the next batch of bases; bytes == 0: the stream has ended"""
        p, n = C.c_void_p(0), C.c_uint64(0)
        check(self._L.jasper_read_feed_next(self._h, C.byref(p), C.byref(n)))
        return (p.value or 0), n.value

    def feed_release(self):
        check(self._L.jasper_read_feed_release(self._h))

    def last_ingest(self):
        """(text bytes parsed on the GPU, text bytes parsed by the host state machine) of the last count_files call"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self._L.jasper_last_ingest(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    INFLATE_KEYS = ("decoders", "accepted", "device_bytes", "host_bytes", "slabs", "members")

    def last_inflate(self):
        """the gzip input of the last count_files / feed call, summed over its files: decoders the device inflater launched, chunks it
        accepted, text bytes inflated on the device and on the host, slabs, members (include/jasper_hip.h jasper_last_inflate)"""
        st = (C.c_uint64 * 6)()
        check(self._L.jasper_last_inflate(self._h, st))
        return dict(zip(self.INFLATE_KEYS, (int(v) for v in st)))

    def count_text(self, text):
        if isinstance(text, str):
            text = text.encode()
        check(self._L.jasper_count_reads_text(self._h, text, len(text)))

    def count_bases(self, bases):
        if isinstance(bases, str):
            bases = bases.encode()
        check(self._L.jasper_count_bases(self._h, bases, len(bases)))

    def count_bases_device(self, dev_ptr, n):
        check(self._L.jasper_count_bases_device(self._h, C.c_void_p(dev_ptr), int(n)))

    def count_timing(self):
        ms = C.c_double(0)
        n = C.c_uint64(0)
        check(self._L.jasper_last_count_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    STAGE_NAMES = {1: ("part1_kernel", "part2_kernel", "region_insert_kernel", "deferred_import3h_kernel"),
                   3: ("part1_kernel", "part2_by_owner_kernel", "region_insert_kernel", "(unused)", "deferred_import3h_kernels"),
                   0: ()}

    def count_stages(self):
        """(ms per kernel stage of the atomic-free counting path the last piece took, launches that took such a path);
        count_path() names the path, STAGE_NAMES[path] the stages"""
        ms = (C.c_double * 8)()
        n = C.c_uint64(0)
        path = C.c_int(0)
        check(self._L.jasper_last_count_stages(self._h, ms, C.byref(n), C.byref(path)))
        self._count_path = path.value
        return list(ms)[:len(self.STAGE_NAMES.get(path.value, ()))] or list(ms)[:5], n.value

    def count_path(self):
        """3 = region lists exchanged between GPUs, 1 = one record per occurrence through partition passes and LDS images, 0 = count_kernel"""
        self.count_stages()
        return self._count_path

    def clear(self):
        check(self._L.jasper_table_clear(self._h))

    def sync(self):
        check(self._L.jasper_table_sync(self._h))

    def info(self):
        k = C.c_int(0)
        slots = C.c_uint64(0)
        distinct = C.c_uint64(0)
        occ = C.c_uint64(0)
        check(self._L.jasper_table_info(self._h, C.byref(k), C.byref(slots), C.byref(distinct), C.byref(occ)))
        return dict(k=k.value, slots=slots.value, distinct=distinct.value, occurrences=occ.value)

    # ---- jellyfish histo ---------------------------------------------------------------------------
    def histogram_is_fused(self):
        """True if the last counting call already produced the histogram (binned while the final counts were written)"""
        return bool(self._L.jasper_histogram_is_fused(self._h))

    def histogram(self):
        out = (C.c_uint64 * 10002)()
        check(self._L.jasper_histogram(self._h, out))
        return list(out)

    def histogram_part(self, part, nparts):
        """multiplicity histogram of the keys of owner partition part/nparts only"""
        out = (C.c_uint64 * 10002)()
        check(self._L.jasper_histogram_part(self._h, int(part), int(nparts), out))
        return list(out)

    def histo_rows(self):
        """non-zero rows (multiplicity, n_distinct) as `jellyfish histo` prints them (JF::sub_commands/histo_main.cc:82-84)"""
        import numpy as np
        out = (C.c_uint64 * 10002)()
        check(self._L.jasper_histogram(self._h, out))
        h = np.frombuffer(out, dtype=np.uint64)
        nz = np.flatnonzero(h[1:]) + 1
        return list(zip(nz.tolist(), h[nz].tolist()))

    # ---- qf[MerDNA(s).get_canonical()] -------------------------------------------------------------
    def lookup(self, strings):
        n = len(strings)
        if n == 0:
            return []
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
        offs = (C.c_int64 * (n + 1))()
        tot = 0
        for i, b in enumerate(bs):
            offs[i] = tot
            tot += len(b)
        offs[n] = tot
        out = (C.c_uint32 * n)()
        check(self._L.jasper_lookup(self._h, b"".join(bs), offs, n, out))
        return list(out)

    # ---- merge support -----------------------------------------------------------------------------
    def export_entries(self):
        """numpy uint64 array [n,3]: mixed-hash hi, lo, count"""
        import numpy as np
        n = C.c_uint64(0)
        check(self._L.jasper_table_export(self._h, C.byref(n), None))
        arr = np.zeros((max(int(n.value), 1), 3), dtype=np.uint64)
        cap = C.c_uint64(arr.shape[0])
        check(self._L.jasper_table_export(self._h, C.byref(cap), arr.ctypes.data_as(C.POINTER(C.c_uint64))))
        return arr[: int(cap.value)]

    def import_entries(self, arr):
        import numpy as np
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        if arr.size == 0:
            return
        check(self._L.jasper_table_import(self._h, arr.ctypes.data_as(C.POINTER(C.c_uint64)), arr.shape[0]))

    def export_device(self):
        n = C.c_uint64(0)
        p = C.c_void_p()
        check(self._L.jasper_table_export_device(self._h, C.byref(n), C.byref(p)))
        return p.value, int(n.value)

    def export_to(self, dev_ptr, cap_entries):
        n = C.c_uint64(0)
        check(self._L.jasper_table_export_to(self._h, C.c_void_p(dev_ptr), int(cap_entries), C.byref(n)))
        return int(n.value)

    def export_packed(self, dev_ptr, cap_entries, part=0, nparts=1):
        """16-byte exchange entries of slot-range partition part/nparts into device memory; returns how many exist"""
        n = C.c_uint64(0)
        check(self._L.jasper_table_export_packed(self._h, C.c_void_p(dev_ptr), int(cap_entries), C.byref(n), int(part), int(nparts)))
        return int(n.value)

    def import_packed(self, dev_ptr, n, mode=0):
        check(self._L.jasper_table_import_packed(self._h, C.c_void_p(dev_ptr), int(n), int(mode)))

    def import_packed_multi(self, dev_ptrs, counts):
        """add several entry lists (device pointers, entry counts) in one sweep over the table"""
        n = len(dev_ptrs)
        ps = (C.c_void_p * n)(*[int(p) for p in dev_ptrs])
        cs = (C.c_uint64 * n)(*[int(c) for c in counts])
        check(self._L.jasper_table_import_packed_multi(self._h, ps, cs, n))

    def reserve(self, min_slots):
        check(self._L.jasper_table_reserve(self._h, int(min_slots)))

    def fit(self, max_load=0.5):
        check(self._L.jasper_table_fit(self._h, float(max_load)))

    # ---- counting as an exchange of region lists (include/jasper_hip.h, jasper_count_exchange_*) -------
    def exchange_plan(self, piece_max, n_owners, records_max=0):
        """None when this table / piece size / k has no exchange geometry, else a dict of buffer sizes"""
        out = (C.c_uint64 * 8)()
        rc = self._L.jasper_count_exchange_plan(self._h, int(piece_max), int(records_max), int(n_owners), out)
        if rc == 1:
            return None
        check(rc)
        names = ("records_per_owner", "counts_per_owner", "deferred_cap", "p1", "p2", "region_bits", "slices", "slice_cap")
        d = dict(zip(names, (int(v) for v in out)))
        d["p2"], d["p2_owner"] = d["p2"] & 0xFF, d["p2"] >> 8      # second-level bits split by the senders / left to the owner's extra pass
        return d

    def exchange_scan(self, d_bases, n, pos, end, piece_max, n_owners, d_deferred, deferred_cap):
        """first pass (returns when it is done): the number of k-mer occurrences found in [pos, end)"""
        rec = C.c_uint64(0)
        check(self._L.jasper_count_exchange_scan(self._h, C.c_void_p(d_bases), int(n), int(pos), int(end), int(piece_max), int(n_owners), C.c_void_p(d_deferred),
                                                 int(deferred_cap), C.byref(rec)))
        return rec.value

    def exchange_partition(self, piece_max, records_max, n_owners, d_send, d_send_counts, d_deferred, deferred_cap):
        check(self._L.jasper_count_exchange_partition(self._h, int(piece_max), int(records_max), int(n_owners), C.c_void_p(d_send), C.c_void_p(d_send_counts),
                                                      C.c_void_p(d_deferred), int(deferred_cap)))

    def exchange_dedupe(self, piece_max, records_max, n_owners, d_send, d_send_counts):
        """the lists of the send buffers deduplicated in place: (records in the fullest list, count bits), or None when the
        geometry has no bits for the counts (nothing done)"""
        mx, cb = C.c_uint32(0), C.c_int(0)
        rc = self._L.jasper_count_exchange_dedupe(self._h, int(piece_max), int(records_max), int(n_owners), C.c_void_p(d_send), C.c_void_p(d_send_counts),
                                                  C.byref(mx), C.byref(cb))
        if rc == 1:
            return None
        check(rc)
        return mx.value, cb.value

    def exchange_insert(self, d_recv, d_recv_counts, piece_max, records_max, n_owners, self_index, d_deferred_all=0, n_deferred_all=0, whole_input=False,
                        slice_cap=0, count_bits=0):
        check(self._L.jasper_count_exchange_insert(self._h, C.c_void_p(d_recv), C.c_void_p(d_recv_counts), int(piece_max), int(records_max), int(n_owners),
                                                   int(self_index), C.c_void_p(d_deferred_all or None), int(n_deferred_all), 1 if whole_input else 0,
                                                   int(slice_cap), int(count_bits)))

    # ---- owner-sharded table (include/jasper_hip.h, "Owner-sharded table") ----------------------------
    def export_owner(self, dev_ptr, cap_entries, n_owners):
        """all entries grouped by owner into device memory (segment o at dev_ptr + o*cap*16); returns the n counts"""
        counts = (C.c_uint64 * int(n_owners))()
        check(self._L.jasper_table_export_owner(self._h, C.c_void_p(dev_ptr), int(cap_entries), int(n_owners), counts))
        return [int(c) for c in counts]

    def ipc_handle(self):
        buf = C.create_string_buffer(64)
        check(self._L.jasper_table_ipc_handle(self._h, buf))
        return buf.raw

    def attach_ipc(self, handles, self_index):
        """handles: list of 64-byte IPC handles in owner order (the entry at self_index is not used)"""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == 64 * len(handles)
        check(self._L.jasper_table_attach_ipc(self._h, blob, len(handles), int(self_index)))

    def attach_tables(self, shards, self_index):
        """shards: the owners' Table objects (same process, same device) in owner order"""
        arr = (C.c_void_p * len(shards))(*[t._h for t in shards])
        check(self._L.jasper_table_attach_tables(self._h, arr, len(shards), int(self_index)))
        self._shard_refs = list(shards)      # keep the owners alive while their slot arrays are read through this table

    def release_retired(self):
        """free slot arrays this table has outgrown after their IPC handles were given out (call once every owner has attached
        to the new ones)"""
        check(self._L.jasper_table_release_retired(self._h))

    def detach(self):
        check(self._L.jasper_table_detach(self._h))
        self._shard_refs = None

    def import_device(self, dev_ptr, n):
        check(self._L.jasper_table_import_device(self._h, C.c_void_p(dev_ptr), int(n)))

    def device_free(self, dev_ptr):
        check(self._L.jasper_device_free(self._h, C.c_void_p(dev_ptr)))

    # ---- one batch through the polisher -------------------------------------------------------------
    def polish_batch(self, seqs, solid_thre, passes, fix=True):
        want_str = any(isinstance(s, str) for s in seqs)       # bytes in -> bytes out (no 1-byte-per-char round trip)
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_polish_batch(self._h, n, cs, lens, int(solid_thre), int(passes), 1 if fix else 0, C.byref(res))
        return self._wrap_result(rc, res, n, want_str)

    def polish_batch_device(self, d_text, offsets, solid_thre, passes, fix=True):
        """chunk records already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the chunk
        texts back to back, offsets the n+1 chunk boundaries.  The polished text stays in HBM (PolishResult.seq_device)
        and is copied to the host on first use of seq_view / seqs."""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_polish_batch_device(self._h, n, ptr, offs, int(solid_thre), int(passes), 1 if fix else 0, C.byref(res))
        return self._wrap_result(rc, res, n, False)

    # ---- dense k-mer report (an extension: no counterpart in the reference) ------------------------------
    def kmer_report(self, seqs, thre):
        """per-sequence counters and runs of unreliable k-mers (count < thre) of `seqs` (str or bytes) -> KmerReport"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_kmer_report(self._h, n, cs, lens, int(thre), C.byref(res))
        return self._wrap_report(rc, res)

    def kmer_report_device(self, d_text, offsets, thre):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_kmer_report_device(self._h, n, ptr, offs, int(thre), C.byref(res))
        return self._wrap_report(rc, res)

    @staticmethod
    def report_tile_windows():
        """windows per tile of the report's scan kernel (runs are stitched across tiles; tests aim at the seams)"""
        return int(_lib.lib().jasper_report_tile_windows())

    # ---- copy-number k-mer spectrum (an extension: no counterpart in the reference) ------------------------
    def spectrum(self, assembly_table):
        """this table as the reads' counts joined on the GPU with `assembly_table` (a whole KmerTable of the same k on the same
        device, the assembly counted into it) -> KmerSpectrum; neither table is modified"""
        import numpy as np
        if not isinstance(assembly_table, KmerTable) or not assembly_table._h:
            raise TypeError("spectrum: the assembly must be an open KmerTable")
        cells = np.zeros((int(self._L.jasper_spectrum_rows()), 10002), dtype=np.uint64)
        secs = C.c_double(0)
        check(self._L.jasper_table_spectrum(self._h, assembly_table._h, cells.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(secs)))
        return KmerSpectrum(cells, secs.value)

    # ---- copy-number scan (an extension: no counterpart in the reference) ---------------------------------
    def _assembly_handle(self, assembly_table, what):
        if not isinstance(assembly_table, KmerTable) or not assembly_table._h:
            raise TypeError("%s: the assembly must be an open KmerTable" % what)
        return assembly_table._h

    def copy_report(self, assembly_table, seqs, thre, peak):
        """this table as the reads' counts, `assembly_table` the assembly's (a whole KmerTable of the same k on the same device):
        per-sequence counters and the runs of windows whose read count supports more (excess) or fewer (deficit) copies than the
        assembly holds, `peak` = the read count of a single-copy k-mer -> CopyReport; neither table is modified"""
        ah = self._assembly_handle(assembly_table, "copy_report")
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_copy_report(self._h, ah, n, cs, lens, int(thre), _peak32(peak), C.byref(res))
        return self._wrap_copyrep(rc, res)

    def copy_report_device(self, assembly_table, d_text, offsets, thre, peak):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        ah = self._assembly_handle(assembly_table, "copy_report_device")
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_copy_report_device(self._h, ah, n, ptr, offs, int(thre), _peak32(peak), C.byref(res))
        return self._wrap_copyrep(rc, res)

    def _wrap_copyrep(self, rc, res):
        try:
            check(rc)
            counts = _counts(self._L.jasper_copyrep_num_seqs, self._L.jasper_copyrep_counts, res, 6)
            runs = _records(self._L.jasper_copyrep_runs, res, _lib.CopyRun, COPYRUN_DTYPE)
            return CopyReport(counts, runs, self._L.jasper_copyrep_seconds(res), bool(self._L.jasper_copyrep_retried(res)))
        finally:
            if res:
                self._L.jasper_copyrep_free(res)

    # ---- both haplotypes of a diploid assembly (an extension: no counterpart in the reference) ------------
    def spectrum_pair(self, asm_table, alt_table):
        """this table as the reads' counts joined on the GPU with `asm_table` and `alt_table` (whole KmerTables of the same k on the
        same device, one haplotype's assembly counted into each) -> PairSpectrum; no table is modified"""
        import numpy as np
        for t, name in ((asm_table, "assembly"), (alt_table, "alt assembly")):
            if not isinstance(t, KmerTable) or not t._h:
                raise TypeError("spectrum_pair: the %s must be an open KmerTable" % name)
        cells = np.zeros((4, 10002), dtype=np.uint64)
        secs = C.c_double(0)
        check(self._L.jasper_table_spectrum_pair(self._h, asm_table._h, alt_table._h, cells.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(secs)))
        return PairSpectrum(cells, secs.value)

    def pair_scan(self, other_table, seqs, thre):
        """this table as the reads' counts, `other_table` the OTHER haplotype's (a whole KmerTable of the same k on the same device),
        `seqs` the sequences of THIS haplotype: per-sequence counters and the runs of windows the other haplotype does not hold,
        solid (the reads hold them `thre` times or more) or weak -> PairScan; neither table is modified"""
        if not isinstance(other_table, KmerTable) or not other_table._h:
            raise TypeError("pair_scan: the other haplotype must be an open KmerTable")
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_pair_scan(self._h, other_table._h, n, cs, lens, int(thre), C.byref(res))
        try:
            check(rc)
            counts = _counts(self._L.jasper_pairscan_num_seqs, self._L.jasper_pairscan_counts, res, 6)
            runs = _records(self._L.jasper_pairscan_runs, res, _lib.PairRun, PAIRRUN_DTYPE)
            return PairScan(counts, runs, self._L.jasper_pairscan_seconds(res), bool(self._L.jasper_pairscan_retried(res)))
        finally:
            if res:
                self._L.jasper_pairscan_free(res)

    # ---- duplication map (an extension: no counterpart in the reference) ----------------------------------
    def dup_map(self, assembly_table, seqs, thre, peak):
        """this table as the reads' counts, `assembly_table` the assembly's (a whole KmerTable of the same k on the same device,
        counted from exactly `seqs`): every window whose k-mer the assembly holds exactly twice paired with the place of the other
        copy, as per-sequence counters and the maximal colinear runs of such pairs; `thre` and `peak` as for copy_report ->
        DupMap; neither table is modified"""
        ah = self._assembly_handle(assembly_table, "dup_map")
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_dup_map(self._h, ah, n, cs, lens, int(thre), _peak32(peak), C.byref(res))
        return self._wrap_dupmap(rc, res)

    def dup_map_device(self, assembly_table, d_text, offsets, thre, peak):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        ah = self._assembly_handle(assembly_table, "dup_map_device")
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_dup_map_device(self._h, ah, n, ptr, offs, int(thre), _peak32(peak), C.byref(res))
        return self._wrap_dupmap(rc, res)

    def _wrap_dupmap(self, rc, res):
        try:
            check(rc)
            counts = _counts(self._L.jasper_dupmap_num_seqs, self._L.jasper_dupmap_counts, res, 7)
            runs = _records(self._L.jasper_dupmap_runs, res, _lib.DupRun, DUPRUN_DTYPE)
            index, scan = C.c_double(0), C.c_double(0)
            check(self._L.jasper_dupmap_seconds(res, C.byref(index), C.byref(scan)))
            return DupMap(counts, runs, (index.value, scan.value), bool(self._L.jasper_dupmap_retried(res)))
        finally:
            if res:
                self._L.jasper_dupmap_free(res)

    # ---- trio hap-mer scan and census (an extension: no counterpart in the reference) ----------------------
    @staticmethod
    def _parent_handle(t, who, what):
        if not isinstance(t, KmerTable) or not t._h:
            raise TypeError("%s: the %s table must be an open KmerTable" % (what, who))
        return t._h

    def hapmer_scan(self, mat, pat, seqs, thre_mat, thre_pat, thre_child=1, child=True):
        """this table as the child's reads, `mat` / `pat` the mother's and the father's (whole KmerTables of the same k on the same
        device): per-sequence counters and the runs of windows whose k-mer only one parent holds (solid there, absent from the
        other, and solid in this table) -> HapmerScan.  child=False: no inheritance filter, this table is not consulted
        (KmerTable.hapmer_scan_parents is the same without a child table at all).  No table is modified"""
        return KmerTable.hapmer_scan_parents(mat, pat, seqs, thre_mat, thre_pat, thre_child, _child=self if child else None)

    @staticmethod
    def hapmer_scan_parents(mat, pat, seqs, thre_mat, thre_pat, thre_child=1, _child=None):
        """the hap-mer scan without a child table: every solid k-mer of one parent that the other lacks is a marker"""
        mh, ph = KmerTable._parent_handle(mat, "maternal", "hapmer_scan"), KmerTable._parent_handle(pat, "paternal", "hapmer_scan")
        ch = KmerTable._parent_handle(_child, "child", "hapmer_scan") if _child is not None else None
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = mat._L.jasper_hapmer_scan(mh, ph, ch, n, cs, lens, _thre32(thre_mat), _thre32(thre_pat), _thre32(thre_child), C.byref(res))
        return mat._wrap_hapscan(rc, res)

    def hapmer_scan_device(self, mat, pat, d_text, offsets, thre_mat, thre_pat, thre_child=1, child=True):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        mh, ph = self._parent_handle(mat, "maternal", "hapmer_scan_device"), self._parent_handle(pat, "paternal", "hapmer_scan_device")
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_hapmer_scan_device(mh, ph, self._h if child else None, n, ptr, offs, _thre32(thre_mat), _thre32(thre_pat), _thre32(thre_child),
                                               C.byref(res))
        return self._wrap_hapscan(rc, res)

    def _wrap_hapscan(self, rc, res):
        try:
            check(rc)
            counts = _counts(self._L.jasper_hapscan_num_seqs, self._L.jasper_hapscan_counts, res, 4)
            runs = _records(self._L.jasper_hapscan_runs, res, _lib.HapRun, HAPRUN_DTYPE)
            return HapmerScan(counts, runs, self._L.jasper_hapscan_seconds(res), bool(self._L.jasper_hapscan_retried(res)))
        finally:
            if res:
                self._L.jasper_hapscan_free(res)

    def hapmer_census(self, mat, pat, asm=None, thre_mat=1, thre_pat=1, thre_child=1, child=True):
        """this table as the child's reads: how many hap-mers each parent has (solid there, absent from the other parent, solid in
        this table), how many of them the assembly's table `asm` holds and how often -> HapmerCensus.  asm=None: found and
        occurrences are 0; child=False: no inheritance filter"""
        return KmerTable.hapmer_census_parents(mat, pat, asm, thre_mat, thre_pat, thre_child, _child=self if child else None)

    @staticmethod
    def hapmer_census_parents(mat, pat, asm=None, thre_mat=1, thre_pat=1, thre_child=1, _child=None):
        """the hap-mer census without a child table"""
        mh, ph = KmerTable._parent_handle(mat, "maternal", "hapmer_census"), KmerTable._parent_handle(pat, "paternal", "hapmer_census")
        ch = KmerTable._parent_handle(_child, "child", "hapmer_census") if _child is not None else None
        ah = KmerTable._parent_handle(asm, "assembly", "hapmer_census") if asm is not None else None
        out = (C.c_uint64 * 6)()
        secs = C.c_double(0)
        check(mat._L.jasper_hapmer_census(mh, ph, ch, ah, _thre32(thre_mat), _thre32(thre_pat), _thre32(thre_child), out, C.byref(secs)))
        v = [int(x) for x in out]
        return HapmerCensus(tuple(v[:3]), tuple(v[3:]), secs.value)

    # ---- a join of tables as a table (an extension: the census's set, kept instead of counted) ------------------
    SELECT_SLOTS_LEAST, SELECT_SLOTS_MOST = 1 << 16, 1 << 26

    @staticmethod
    def select(src, absent, solid=None, thre_src=1, thre_solid=1):
        """the keys of `src` with a count of at least thre_src that `absent` does not hold and (with `solid`) that `solid` holds at least
        thre_solid times, with their counts in src, as a NEW table on src's device (include/jasper_hip.h: jasper_table_select) ->
        (KmerTable, stats); stats = dict of candidates, in_absent, not_solid, selected and seconds (device time of the select sweeps).
        The caller closes the table.  It starts at 1/16 of src's distinct keys in slots, at least 2^16 and at most 2^26, grows as any
        table does while the pieces are imported, and is cut to a load of at most 0.5 at the end."""
        sh, ah = KmerTable._parent_handle(src, "source", "select"), KmerTable._parent_handle(absent, "absent", "select")
        rh = KmerTable._parent_handle(solid, "solid", "select") if solid is not None else None
        slots = min(max(src.info()["distinct"] // 16, KmerTable.SELECT_SLOTS_LEAST), KmerTable.SELECT_SLOTS_MOST)
        dst = KmerTable(src.k, min_slots=slots, device=src.device)
        try:
            out = (C.c_uint64 * 4)()
            secs = C.c_double(0)
            check(src._L.jasper_table_select(dst._h, sh, ah, rh, _thre32(thre_src), _thre32(thre_solid), out, C.byref(secs)))
            dst.fit()
        except BaseException:
            dst.close()
            raise
        v = [int(x) for x in out]
        return dst, dict(candidates=v[0], in_absent=v[1], not_solid=v[2], selected=v[3], seconds=secs.value)

    @staticmethod
    def subtract(src, minus):
        """src - minus as a NEW table on src's device (include/jasper_hip.h: jasper_table_subtract): the keys of `src` whose 64-bit count
        exceeds their count in `minus`, each with the difference -> (KmerTable, stats); stats = dict of swept, matched, dropped,
        underflow, kept, missing (= the distinct keys of minus - matched) and seconds (device time of the sweeps).  underflow or missing
        above 0: minus is no sub-multiset of src; the table comes back all the same and the caller decides.  Neither source is
        modified; the caller closes the table.  It is sized for src's distinct keys and cut to a load of at most 0.5 at the end."""
        sh, mh = KmerTable._parent_handle(src, "source", "subtract"), KmerTable._parent_handle(minus, "minus", "subtract")
        dst = KmerTable(src.k, min_slots=max(2 * src.info()["distinct"], KmerTable.SELECT_SLOTS_LEAST), device=src.device)
        try:
            out = (C.c_uint64 * 5)()
            secs = C.c_double(0)
            check(src._L.jasper_table_subtract(dst._h, sh, mh, out, C.byref(secs)))
            dst.fit()
        except BaseException:
            dst.close()
            raise
        v = [int(x) for x in out]
        return dst, dict(swept=v[0], matched=v[1], dropped=v[2], underflow=v[3], kept=v[4], missing=minus.info()["distinct"] - v[1], seconds=secs.value)

    # ---- the reads of chosen bins counted into tables of their own (an extension: what triobin --write-jf is made of) ----
    @staticmethod
    def _sink_args(sinks, what):
        """sinks: pairs (KmerTable, bins) with bins the bin codes the table takes (an iterable of 0 .. 2) or their mask as an int ->
        (n, handles, masks, out, seconds) for the C call"""
        sinks = list(sinks)
        handles = (C.c_void_p * max(len(sinks), 1))(*(KmerTable._parent_handle(t, "sink", what).value for t, _ in sinks))
        masks = (C.c_uint32 * max(len(sinks), 1))()
        for i, (_, bins) in enumerate(sinks):
            m = int(bins) if isinstance(bins, int) else sum(1 << int(b) for b in set(bins))
            if not 0 <= m <= 0xFFFFFFFF:
                raise ValueError("%s: a sink's bins must be codes 0 .. 2 or their mask" % what)
            masks[i] = m
        return len(sinks), handles, masks, (C.c_uint64 * (3 * max(len(sinks), 1)))(), (C.c_double * (2 * max(len(sinks), 1)))()

    @staticmethod
    def _sink_stats(n, out, secs):
        return [dict(reads=int(out[3 * i]), bases=int(out[3 * i + 1]), occurrences=int(out[3 * i + 2]), gather_seconds=secs[2 * i], count_seconds=secs[2 * i + 1])
                for i in range(n)]

    @staticmethod
    def _codes(codes, n, what):
        import numpy as np
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        if codes.ndim != 1 or len(codes) != n:
            raise ValueError("%s: codes must hold one bin code per read" % what)
        return codes

    @staticmethod
    def count_binned(reads, codes, sinks):
        """the reads of chosen bins counted into tables (include/jasper_hip.h: jasper_count_binned).  reads: as read_bins takes them;
        codes: one bin code 0 .. 2 per read; sinks: up to three pairs (KmerTable, bins) -- the table is added the canonical k-mers of
        the reads whose code is in bins (an iterable of codes, or their mask), no k-mer spanning two reads -> a dict per sink: reads,
        bases, occurrences gathered, gather_seconds (device time of the gather kernel), count_seconds (wall time of the counting)"""
        import numpy as np
        buf, offs = KmerTable._packed_reads(reads)
        codes = KmerTable._codes(codes, len(offs) - 1, "count_binned")
        ptr = C.c_char_p(buf) if isinstance(buf, bytes) else C.c_void_p(buf.ctypes.data if buf.size else None)
        n, handles, masks, out, secs = KmerTable._sink_args(sinks, "count_binned")
        check(_lib.lib().jasper_count_binned(n, handles, masks, len(offs) - 1, ptr, C.c_void_p(offs.ctypes.data), C.c_void_p(codes.ctypes.data) if len(codes) else None,
                                             out, secs))
        return KmerTable._sink_stats(n, out, secs)

    @staticmethod
    def count_binned_device(d_text, offsets, codes, sinks):
        """the same for reads already in HBM on the sinks' device: d_text is a device pointer (int) or an object with .data_ptr() holding
        the reads back to back, complete when the call is made; offsets the n+1 boundaries (host)"""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1:
            raise ValueError("count_binned_device: offsets must hold n+1 boundaries")
        codes = KmerTable._codes(codes, len(offs) - 1, "count_binned_device")
        ptr = d_text.data_ptr() if hasattr(d_text, "data_ptr") else int(d_text)
        n, handles, masks, out, secs = KmerTable._sink_args(sinks, "count_binned_device")
        check(_lib.lib().jasper_count_binned_device(n, handles, masks, len(offs) - 1, C.c_void_p(ptr), C.c_void_p(offs.ctypes.data),
                                                    C.c_void_p(codes.ctypes.data) if len(codes) else None, out, secs))
        return KmerTable._sink_stats(n, out, secs)

    @staticmethod
    def count_binned_workspace(mat, pat, n_records, codes, sinks):
        """the same for the packed sequences the last read_bins_text / GzText.bins call on (mat, pat) left in mat's workspace (--reader
        device: no sequence visits the host).  n_records is what that call returned; pat may be None; neither may be a sink"""
        mh = KmerTable._parent_handle(mat, "maternal", "count_binned_workspace")
        ph = KmerTable._parent_handle(pat, "paternal", "count_binned_workspace") if pat is not None else None
        codes = KmerTable._codes(codes, int(n_records), "count_binned_workspace")
        n, handles, masks, out, secs = KmerTable._sink_args(sinks, "count_binned_workspace")
        check(mat._L.jasper_read_text_count(mh, ph, int(n_records), C.c_void_p(codes.ctypes.data) if len(codes) else None, n, handles, masks, out, secs))
        return KmerTable._sink_stats(n, out, secs)

    # ---- trio read binning (an extension: the hap-mer scan's probes over a packed batch of reads) ----------
    @staticmethod
    def _packed_reads(reads):
        """reads as one flat buffer and its boundaries: a list of bytes / str, or a pair (buffer, offsets) with the buffer bytes or
        np.uint8 and the offsets n+1 integers -> (bytes-like or np.uint8 array, np.int64[n+1], contiguous)"""
        import numpy as np
        if isinstance(reads, tuple) and len(reads) == 2 and not isinstance(reads[1], (bytes, str)):
            buf, offs = reads
            if isinstance(buf, str):
                buf = buf.encode("latin-1")
            if not isinstance(buf, bytes):
                buf = np.ascontiguousarray(buf)
                if buf.dtype != np.uint8 or buf.ndim != 1:
                    raise TypeError("read_bins: the buffer must be bytes or a one-dimensional np.uint8 array")
            offs = np.ascontiguousarray(offs, dtype=np.int64)
            if offs.ndim != 1 or len(offs) < 1:
                raise ValueError("read_bins: offsets must hold n+1 boundaries")
            if len(offs) > 1 and (int(offs[0]) < 0 or int(offs[-1]) > len(buf)):
                raise ValueError("read_bins: offsets reach outside the buffer")
            return buf, offs
        bs = [s.encode("latin-1") if isinstance(s, str) else (s if isinstance(s, bytes) else bytes(s)) for s in reads]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            np.cumsum([len(b) for b in bs], out=offs[1:])
        return b"".join(bs), offs

    @staticmethod
    def _read_bins_call(fn, mat, pat, text_ptr, offs, thre_mat, thre_pat, what):
        import numpy as np
        mh, ph = KmerTable._parent_handle(mat, "maternal", what), KmerTable._parent_handle(pat, "paternal", what)
        n = len(offs) - 1
        om, op = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        secs = C.c_double(0)
        check(fn(mh, ph, n, text_ptr, C.c_void_p(offs.ctypes.data), _thre32(thre_mat), _thre32(thre_pat), C.c_void_p(om.ctypes.data), C.c_void_p(op.ctypes.data),
                 C.byref(secs)))
        return ReadBins(om, op, secs.value)

    @staticmethod
    def read_bins(mat, pat, reads, thre_mat, thre_pat):
        """`mat` / `pat` the mother's and the father's whole KmerTables (one k, one device): per read the windows whose k-mer is solid
        in one parent (count >= its threshold) and absent from the other -> ReadBins.  reads: a list of bytes / str, or a pair
        (buffer, offsets) of the reads back to back (bytes or np.uint8) and their n+1 boundaries (np.int64).  No table is modified"""
        import numpy as np
        buf, offs = KmerTable._packed_reads(reads)
        ptr = C.c_char_p(buf) if isinstance(buf, bytes) else C.c_void_p(buf.ctypes.data)
        if isinstance(buf, np.ndarray) and buf.size == 0:
            ptr = None
        return KmerTable._read_bins_call(mat._L.jasper_read_bins if isinstance(mat, KmerTable) else None, mat, pat, ptr, offs, thre_mat, thre_pat, "read_bins")

    @staticmethod
    def read_bins_device(mat, pat, d_text, offsets, thre_mat, thre_pat):
        """the same for reads already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the reads back to
        back, offsets the n+1 boundaries (host)"""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1:
            raise ValueError("read_bins_device: offsets must hold n+1 boundaries")
        ptr = d_text.data_ptr() if hasattr(d_text, "data_ptr") else int(d_text)
        return KmerTable._read_bins_call(mat._L.jasper_read_bins_device if isinstance(mat, KmerTable) else None, mat, pat, C.c_void_p(ptr), offs, thre_mat, thre_pat,
                                         "read_bins_device")

    @staticmethod
    def read_bins_text(mat, pat, buf, eof, fmt, thre_mat, thre_pat, want_seq=False):
        """the same from raw file text: buf (bytes or np.uint8) begins at a record's first byte, fmt is "fastq" or "fasta", eof says
        whether buf ends the file.  The GPU finds the lines, verifies the records, packs the sequences and bins them -> ReadText; the
        caller carries buf[used:] over to the next chunk.  A malformed chunk is no error: ReadText.malformed, nothing binned"""
        import numpy as np
        if fmt not in READ_TEXT_FORMATS:
            raise ValueError("read_bins_text: fmt must be 'fastq' or 'fasta'")
        if not isinstance(buf, bytes):
            buf = np.ascontiguousarray(buf)
            if buf.dtype != np.uint8 or buf.ndim != 1:
                raise TypeError("read_bins_text: the buffer must be bytes or a one-dimensional np.uint8 array")
        mh, ph = KmerTable._parent_handle(mat, "maternal", "read_bins_text"), KmerTable._parent_handle(pat, "paternal", "read_bins_text")
        ptr = C.c_char_p(buf) if isinstance(buf, bytes) else C.c_void_p(buf.ctypes.data if buf.size else None)
        used, n, bad, status, secs = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0), (C.c_double * 2)()
        L = mat._L
        check(L.jasper_read_text_bins(mh, ph, ptr, len(buf), 1 if eof else 0, READ_TEXT_FORMATS[fmt], _thre32(thre_mat), _thre32(thre_pat), C.byref(used), C.byref(n),
                                      C.byref(status), C.byref(bad), secs))
        r = ReadText(used.value, n.value, status.value != 0, bad.value, secs[1], secs[0])
        if r.malformed:
            return r
        return _fetch_records(L, mh, r, want_seq)

    def gz_text(self, path):
        """a gzip text session on this table (the maternal one of the binning calls): the .gz file inflated on the GPU -> GzText.  Raises
        when the file is not for the device inflater (no gzip header, not a regular file): the caller reads it the ordinary way"""
        return GzText(self, path)

    def deflate_bgzf(self, text, out=None):
        """text (bytes or np.uint8) -> (its BGZF members as np.uint8, one per 65280 bytes, without the empty member that ends a file;
        the counters DEFLATE_COUNTERS as a dict; device seconds of the kernels).  out: a contiguous np.uint8 array of at least
        deflate_bound(len(text)) bytes to write into (the result is a view of it)"""
        import numpy as np
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text
        if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
            raise TypeError("deflate_bgzf: the text must be bytes or a contiguous one-dimensional np.uint8 array")
        room = deflate_bound(len(buf))
        if out is None:
            out = np.empty(max(room, 1), dtype=np.uint8)
        if out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous or len(out) < room:
            raise ValueError("deflate_bgzf: out must be a contiguous np.uint8 array of at least deflate_bound(len(text)) bytes")
        vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
        nb, cnt, secs = C.c_int64(0), (C.c_uint64 * 6)(), C.c_double(0)
        check(self._L.jasper_deflate_bgzf(self._h, vp(buf) if buf.size else None, len(buf), vp(out), len(out), C.byref(nb), cnt, C.byref(secs)))
        return out[:nb.value], dict(zip(DEFLATE_COUNTERS, (int(v) for v in cnt))), secs.value

    def route_text(self, text, bounds, bins, first, check_from=0, out=None, gz=False):
        """text (bytes or np.uint8) cut by bounds[n_seg + 1] into segments with bin codes bins[n_seg] (0..2) -> RoutedText: each bin's
        segments back to back, and the segments i >= check_from that hold a byte and do not begin with `first`.  gz=True: each bin's
        bytes come back as BGZF members, compressed on the GPU (out: room for deflate_bound(len(text)) bytes each)"""
        import numpy as np
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text
        if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
            raise TypeError("route_text: the text must be bytes or a contiguous one-dimensional np.uint8 array")
        return _route_call(self._L, self._h, None, buf, len(buf), len(buf), bounds, bins, first, check_from, out, gz)

    # ---- variant scan (an extension: the reference acts on such sites inside its walk and reports nothing) --
    def variant_scan(self, seqs, thre):
        """the positions of the sequences where the reads hold a solid single-base alternative (count of all k covering windows
        >= thre >= 1) -> VariantScan; the table is not modified"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_variant_scan(self._h, n, cs, lens, int(thre), C.byref(res))
        return self._wrap_varscan(rc, res)

    def variant_scan_device(self, d_text, offsets, thre):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_variant_scan_device(self._h, n, ptr, offs, int(thre), C.byref(res))
        return self._wrap_varscan(rc, res)

    # ---- indel scan (an extension: the length-changing half of the variant scan, from the same dense scan) --
    def indel_scan(self, seqs, thre, max_len=4, mixed=False, clusters=0):
        """the same-base insertions and the deletions of up to max_len (1..16) bytes that the reads hold against the sequences, and
        the substitution sites of variant_scan with them (thre >= 1, k >= 2) -> IndelScan; with `mixed` also the insertions of mixed
        bases (IndelScan.mixed); with `clusters` = N (1..64; 0: off) also the clusters of heterozygous differences less than k apart,
        as replacements of up to N bytes by up to N bases (IndelScan.clusters); the table is not modified"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        if clusters:
            rc = self._L.jasper_indel_scan_clusters(self._h, n, cs, lens, int(thre), int(max_len), int(bool(mixed)), int(clusters), C.byref(res))
            return self._wrap_indelscan(rc, res, mixed, True)
        fn = self._L.jasper_indel_scan_mixed if mixed else self._L.jasper_indel_scan
        rc = fn(self._h, n, cs, lens, int(thre), int(max_len), C.byref(res))
        return self._wrap_indelscan(rc, res, mixed)

    def indel_scan_device(self, d_text, offsets, thre, max_len=4, mixed=False, clusters=0):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        if clusters:
            rc = self._L.jasper_indel_scan_clusters_device(self._h, n, ptr, offs, int(thre), int(max_len), int(bool(mixed)), int(clusters), C.byref(res))
            return self._wrap_indelscan(rc, res, mixed, True)
        fn = self._L.jasper_indel_scan_mixed_device if mixed else self._L.jasper_indel_scan_device
        rc = fn(self._h, n, ptr, offs, int(thre), int(max_len), C.byref(res))
        return self._wrap_indelscan(rc, res, mixed)

    # ---- compound scan (an extension: what the reads hold in place of differences that hide each other) ------
    def compound_scan(self, seqs, thre, max_len=64):
        """the replacements of up to max_len (1..64) bases that the reads hold for the runs of unreliable k-mers that two or more
        differences less than k apart leave, and the kmer_report of the same input (thre >= 1, k >= 2) -> CompoundScan; the table is
        not modified"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_compound_scan(self._h, n, cs, lens, int(thre), int(max_len), C.byref(res))
        return self._wrap_compscan(rc, res)

    def compound_scan_device(self, d_text, offsets, thre, max_len=64):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_compound_scan_device(self._h, n, ptr, offs, int(thre), int(max_len), C.byref(res))
        return self._wrap_compscan(rc, res)

    @staticmethod
    def compound_front():
        """the most prefixes of one length the compound search keeps (a wider level makes the site complex)"""
        return int(_lib.lib().jasper_compound_front())

    def _wrap_compscan(self, rc, res):
        try:
            check(rc)
            counts = _counts(self._L.jasper_compscan_num_seqs, self._L.jasper_compscan_counts, res, 5)
            recs = _records(self._L.jasper_compscan_records, res, _lib.Compound, COMPOUND_DTYPE)
            nl = C.c_uint64(0)
            check(self._L.jasper_compscan_lookups(res, C.byref(nl)))
            search, total = C.c_double(0), C.c_double(0)
            check(self._L.jasper_compscan_seconds(res, C.byref(search), C.byref(total)))
            rep = self._read_report(C.c_void_p(self._L.jasper_compscan_report(res)))      # (owned by res: read, not freed)
            return CompoundScan(counts, recs, rep, total.value, search.value, int(nl.value), bool(self._L.jasper_compscan_retried(res)))
        finally:
            if res:
                self._L.jasper_compscan_free(res)

    # ---- gap scan (an extension: what the reads hold in place of scaffold gaps and long runs of unreliable k-mers) ------
    def gap_scan(self, seqs, thre, max_len=1000, max_trim=None, long_runs=False):
        """the fills of up to max_len (0..4096) bases that the reads hold for the N gaps of the sequences and, with long_runs, for the
        runs of unreliable k-mers that replace more than 64 bytes, and the kmer_report of the same input (thre >= 1, k >= 2; max_trim =
        the most unreliable bases between a flank and the gap, None: k) -> GapScan; the table is not modified"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_gap_scan(self._h, n, cs, lens, _thre32(thre), int(max_len), int(self.k if max_trim is None else max_trim), int(bool(long_runs)), C.byref(res))
        return self._wrap_gapscan(rc, res, True)

    def gap_scan_device(self, d_text, offsets, thre, max_len=1000, max_trim=None, long_runs=False):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_gap_scan_device(self._h, n, ptr, offs, _thre32(thre), int(max_len), int(self.k if max_trim is None else max_trim), int(bool(long_runs)),
                                            C.byref(res))
        return self._wrap_gapscan(rc, res, True)

    def gap_search(self, seqs, thre, max_len, sites):
        """the search alone on the caller's sites: a structured array (GAP_SITE_DTYPE; see make_gap_sites) or [(seq, a, q[, ref_min])] in
        (seq, a) order with k-1 <= a <= q <= n-(k-1); anything else raises and launches nothing -> GapScan without a report"""
        import numpy as np
        n, cs, lens = _seq_args(seqs)
        arr = np.ascontiguousarray(sites if hasattr(sites, "dtype") else make_gap_sites(sites), dtype=GAP_SITE_DTYPE)
        res = C.c_void_p()
        rc = self._L.jasper_gap_search(self._h, n, cs, lens, _thre32(thre), int(max_len), C.c_void_p(arr.ctypes.data if len(arr) else None), len(arr), C.byref(res))
        return self._wrap_gapscan(rc, res, False)

    @staticmethod
    def gap_front():
        """the most strings of one length the gap search keeps (a wider level makes the site complex)"""
        return int(_lib.lib().jasper_gap_front())

    @staticmethod
    def gap_max_records():
        """the most fills of one site the gap search lists (more make the site complex)"""
        return int(_lib.lib().jasper_gap_max_records())

    @staticmethod
    def gap_max_len():
        """the longest fill the gap search can be asked for"""
        return int(_lib.lib().jasper_gap_max_len())

    def _wrap_gapscan(self, rc, res, with_report):
        try:
            check(rc)
            counts = _counts(self._L.jasper_gapscan_num_seqs, self._L.jasper_gapscan_counts, res, 9)
            sites = _records(self._L.jasper_gapscan_sites, res, _lib.GapSite, GAP_SITE_DTYPE)
            recs = _records(self._L.jasper_gapscan_records, res, _lib.GapFill, GAP_FILL_DTYPE)
            bp, bn = C.c_void_p(), C.c_uint64(0)
            check(self._L.jasper_gapscan_bases(res, C.byref(bp), C.byref(bn)))
            bases = C.string_at(bp, bn.value) if bn.value else b""
            nl = C.c_uint64(0)
            check(self._L.jasper_gapscan_lookups(res, C.byref(nl)))
            search, runs, total = C.c_double(0), C.c_double(0), C.c_double(0)
            check(self._L.jasper_gapscan_seconds(res, C.byref(search), C.byref(runs), C.byref(total)))
            rep = self._read_report(C.c_void_p(self._L.jasper_gapscan_report(res))) if with_report else None      # (owned by res: read, not freed)
            return GapScan(counts, sites, recs, bases, rep, total.value, search.value, runs.value, int(nl.value), bool(self._L.jasper_gapscan_retried(res)))
        finally:
            if res:
                self._L.jasper_gapscan_free(res)

    # ---- repair (an extension: the scans' error records applied to the text on the GPU, in rounds) ------------
    def repair(self, seqs, thre, indel_max_len=4, compound_max_len=64, rounds=3):
        """the error records of indel_scan(mixed=True) and compound_scan applied to the sequences, in at most `rounds` (1..8) rounds of
        scan, select and apply (thre >= 1, k >= 2) -> Repair; the table is not modified"""
        n, cs, lens = _seq_args(seqs)
        res = C.c_void_p()
        rc = self._L.jasper_repair(self._h, n, cs, lens, _thre32(thre), int(indel_max_len), int(compound_max_len), int(rounds), C.byref(res))
        return self._wrap_repaired(rc, res)

    def repair_device(self, d_text, offsets, thre, indel_max_len=4, compound_max_len=64, rounds=3):
        """the same for sequences already in HBM: d_text is a device pointer (int) or an object with .data_ptr() holding the
        sequences back to back, offsets the n+1 boundaries; that text is not written"""
        n, ptr, offs = _text_args(d_text, offsets)
        res = C.c_void_p()
        rc = self._L.jasper_repair_device(self._h, n, ptr, offs, _thre32(thre), int(indel_max_len), int(compound_max_len), int(rounds), C.byref(res))
        return self._wrap_repaired(rc, res)

    def apply_edits(self, seqs, edits):
        """the sequences with `edits` applied by the repair stage's kernel -> list of bytes.  edits: a structured array (EDIT_DTYPE; see
        make_edits) ordered by (seq, pos), every edit inside its sequence and at least one byte after the edit before it; anything else
        raises and launches nothing"""
        import numpy as np
        n, cs, lens = _seq_args(seqs)
        arr = np.ascontiguousarray(edits, dtype=EDIT_DTYPE)
        res = C.c_void_p()
        rc = self._L.jasper_apply_edits(self._h, n, cs, lens, C.c_void_p(arr.ctypes.data if len(arr) else None), len(arr), C.byref(res))
        return self._wrap_repaired(rc, res).seqs

    def apply_edits_device(self, d_text, offsets, edits):
        """the same for sequences already in HBM (that text is not written) -> list of bytes"""
        import numpy as np
        n, ptr, offs = _text_args(d_text, offsets)
        arr = np.ascontiguousarray(edits, dtype=EDIT_DTYPE)
        res = C.c_void_p()
        rc = self._L.jasper_apply_edits_device(self._h, n, ptr, offs, C.c_void_p(arr.ctypes.data if len(arr) else None), len(arr), C.byref(res))
        return self._wrap_repaired(rc, res).seqs

    @staticmethod
    def repair_tile_bytes():
        """output bytes per workgroup of the repair stage's apply kernel (tests aim at the seams)"""
        return int(_lib.lib().jasper_repair_tile_bytes())

    def _wrap_repaired(self, rc, res):
        try:
            check(rc)
            seqs = []
            for i in range(self._L.jasper_repaired_num_seqs(res)):
                p, ln = C.c_void_p(), C.c_int64(0)
                check(self._L.jasper_repaired_seq(res, i, C.byref(p), C.byref(ln)))
                seqs.append(C.string_at(p, ln.value) if ln.value else b"")
            edits = _records(self._L.jasper_repaired_edits, res, _lib.Edit, EDIT_DTYPE)
            rp = C.POINTER(_lib.RepairRound)()
            rn = C.c_uint64(0)
            check(self._L.jasper_repaired_rounds(res, C.byref(rp), C.byref(rn)))
            rounds = [(int(rp[i].records), int(rp[i].accepted), int(rp[i].conflicts), int(rp[i].ambiguous), int(rp[i].unreliable_before),
                       int(rp[i].unreliable_after)) for i in range(rn.value)]
            before = self._read_report(C.c_void_p(self._L.jasper_repaired_before(res)))      # (owned by res: read, not freed)
            after = self._read_report(C.c_void_p(self._L.jasper_repaired_after(res)))
            ap, tot = C.c_double(0), C.c_double(0)
            check(self._L.jasper_repaired_seconds(res, C.byref(ap), C.byref(tot)))
            return Repair(seqs, edits, rounds, before, after, tot.value, ap.value)
        finally:
            if res:
                self._L.jasper_repaired_free(res)

    def _read_mixed(self, res):
        counts = _counts(self._L.jasper_indelscan_num_seqs, self._L.jasper_indelscan_mixed_counts, res, 3)
        recs = _records(self._L.jasper_indelscan_mixed_records, res, _lib.MixedIns, MIXED_DTYPE)
        nl = C.c_uint64(0)
        check(self._L.jasper_indelscan_mixed_lookups(res, C.byref(nl)))
        return MixedInsertions(counts, recs, self._L.jasper_indelscan_mixed_seconds(res), int(nl.value), bool(self._L.jasper_indelscan_mixed_retried(res)))

    def _read_clusters(self, res):
        counts = _counts(self._L.jasper_indelscan_num_seqs, self._L.jasper_indelscan_cluster_counts, res, 4)
        recs = _records(self._L.jasper_indelscan_cluster_records, res, _lib.HetCluster, HET_CLUSTER_DTYPE)
        nl = C.c_uint64(0)
        check(self._L.jasper_indelscan_cluster_lookups(res, C.byref(nl)))
        return HetClusters(counts, recs, self._L.jasper_indelscan_cluster_seconds(res), int(nl.value), bool(self._L.jasper_indelscan_cluster_retried(res)))

    def _wrap_indelscan(self, rc, res, mixed=False, clusters=False):
        try:
            check(rc)
            counts = _counts(self._L.jasper_indelscan_num_seqs, self._L.jasper_indelscan_counts, res, 4)
            recs = _records(self._L.jasper_indelscan_records, res, _lib.Indel, INDEL_DTYPE)
            nl = C.c_uint64(0)
            check(self._L.jasper_indelscan_lookups(res, C.byref(nl)))
            var = self._read_varscan(C.c_void_p(self._L.jasper_indelscan_variants(res)))      # (owned by res: read, not freed)
            return IndelScan(counts, recs, var, self._L.jasper_indelscan_seconds(res), self._L.jasper_indelscan_check_seconds(res), int(nl.value),
                             bool(self._L.jasper_indelscan_retried(res)), self._read_mixed(res) if mixed else None, self._read_clusters(res) if clusters else None)
        finally:
            if res:
                self._L.jasper_indelscan_free(res)

    def _wrap_varscan(self, rc, res):
        try:
            check(rc)
            return self._read_varscan(res)
        finally:
            if res:
                self._L.jasper_varscan_free(res)

    def _read_varscan(self, res):
        counts = _counts(self._L.jasper_varscan_num_seqs, self._L.jasper_varscan_counts, res, 3)
        recs = _records(self._L.jasper_varscan_records, res, _lib.Variant, VARIANT_DTYPE)
        nc = C.c_uint64(0)
        check(self._L.jasper_varscan_candidates(res, C.byref(nc)))
        return VariantScan(counts, recs, int(nc.value), self._L.jasper_varscan_seconds(res), bool(self._L.jasper_varscan_retried(res)))

    def _wrap_report(self, rc, res):
        try:
            check(rc)
            return self._read_report(res)
        finally:
            if res:
                self._L.jasper_report_free(res)

    def _read_report(self, res):
        counts = _counts(self._L.jasper_report_num_seqs, self._L.jasper_report_counts, res, 4)
        runs = _records(self._L.jasper_report_runs, res, _lib.KmerRun, KMERRUN_DTYPE)
        return KmerReport(counts, runs, self._L.jasper_report_seconds(res), bool(self._L.jasper_report_retried(res)))

    @staticmethod
    def polish_cut_geometry(k):
        """{TMIN, CMIN, CLEAN_CELL, W, M} of the polisher's segment cuts for this k (tests restate the cut rule from these)"""
        out = (C.c_int64 * 5)()
        check(_lib.lib().jasper_polish_cut_geometry(int(k), out))
        return dict(zip(("TMIN", "CMIN", "CLEAN_CELL", "W", "M"), (int(v) for v in out)))

    def _wrap_result(self, rc, res, n, want_str):
        try:
            check(rc)
            aux = []
            for i in range(n):
                ap = C.c_void_p()
                an = C.c_uint64(0)
                check(self._L.jasper_result_aux(res, i, C.byref(ap), C.byref(an)))
                aux.append(C.string_at(ap, an.value) if an.value else b"")
            raw = _records(self._L.jasper_result_records, res, FixRec, FIXREC_DTYPE)
            qv = (C.c_int64 * 4)()
            check(self._L.jasper_result_qv(res, qv))
            nl = C.c_uint64(0)
            check(self._L.jasper_result_lookups(res, C.byref(nl)))
            secs = self._L.jasper_result_seconds(res)
            nseg, nredo = C.c_uint64(0), C.c_uint64(0)
            check(self._L.jasper_result_segments(res, C.byref(nseg), C.byref(nredo)))
            pr = PolishResult(self._L, res, n, want_str, raw, aux, tuple(qv), nl.value, secs)
            res = None   # owned by the PolishResult from here on
            pr.segments, pr.respeculated = nseg.value, nredo.value
            pr.retried = bool(self._L.jasper_result_retried(pr._h))
            return pr
        finally:
            if res:
                self._L.jasper_result_free(res)
