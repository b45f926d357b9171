"""Trio read binning: the child's reads sorted into maternal, paternal and unknown by the parental hap-mers they carry.

    python -m jasper_amd.triobin -r 'child reads...' (--mat 'files' | --mat-jf db.jf) (--pat 'files' | --pat-jf db.jf)
                                 [-k 37] [--mat-threshold N] [--pat-threshold N] [--min-markers N] [--paired] [--per-read] [--write-reads]
                                 [--write-jf] [--write-gz] [--deflate host|device] [--batch-bases N] [--reader host|device] [--gz host|device]
                                 [--route host|device] [--marker-tables] [-o PREFIX] [--device D]
    python -m jasper_amd.triobin -r 'reads...' --hap1 hap1.fa --hap2 hap2.fa [--markers solid|all] [--child-threshold N] [--child-jf db.jf]
                                 [every flag above but the parents' six]

An extension (the reference has no such tool), and the cure for what `--hapmers` only shows: a polisher that repairs toward the reads'
solid k-mers can move a het site of a phased assembly onto the other haplotype, which hapmers.tsv lists as switches in its `after` row.
TrioCanu-style binning prevents it: each haplotype is polished with the reads that belong to it.

    python -m jasper_amd.triobin -r 'child.fq' --mat 'mat.fq' --pat 'pat.fq' --write-reads -o trio
    jasper.sh -a hap1.fa -r 'trio.mat.child.fq trio.unknown.child.fq' ...
    jasper.sh -a hap2.fa -r 'trio.pat.child.fq trio.unknown.child.fq' ...

The parents.  The mother's and the father's reads are counted into two whole tables on one GPU, or their Jellyfish databases are loaded
(--mat-jf / --pat-jf; a database's header decides k, and both parents must have one k).  A marker (hap-mer) is a k-mer that is solid in
one parent -- count >= that parent's threshold, --mat-threshold / --pat-threshold or what its histogram gives -- and has count 0 in the
other.  M_total and P_total are how many of them each parent has (KmerTable.hapmer_census_parents); when either is 0 the run ends with
exit status 1.  All of this is extensions.open_parents, with the messages of `--hapmers`.

--marker-tables.  After the parents are opened and given thresholds, the two hap-mer sets are MATERIALISED as tables of their own
(KmerTable.select: the mother's keys with count >= her threshold that the father does not hold, and the mirror), the parental tables
are closed -- tens of GB on a human trio, for two small tables -- M_total and P_total are the selects' counts, and the reads are binned
against the two marker tables with thresholds 1.  Every output file and both log lines are byte for byte what the run without the flag
writes; JASPER_AMD_TIMING=1 adds one line with both selects' device seconds and their four counters.

Two haplotype assemblies instead of parents (--hap1 hap1.fa --hap2 hap2.fa; the parents' six options are refused beside them).  Both
FASTA files are read as kmerqc reads -a and --alt and counted into tables (extensions.assembly_table).  A marker of hap1 is a k-mer hap1
holds and hap2 does not and -- with --markers solid, the default -- that the READS hold at least --child-threshold times: an assembly
ERROR is private to its haplotype too (kmerqc --alt calls it private_weak), and as a marker it would inflate that haplotype's total and
skew the rule toward the cleaner one.  For that the reads are counted first (as kmerqc counts -r), or --child-jf db.jf is loaded (its
header decides k); the threshold is --child-threshold or what the solid-k-mer rule derives from the histogram, and a histogram that
gives none ends the run with exit status 1 and a message that asks for the flag.  --markers all takes every private k-mer and counts
nothing.  Two selects make the marker tables (M' = select(hap1, hap2, reads, 1, threshold), P' its mirror), the three source tables are
closed, M_total and P_total are the selected counts, and everything below runs on (M', P', 1, 1) -- every reader, --gz, --route and
--deflate combination.  The bins are hap1, hap2 and unknown in the file names, in both tables (columns hap1_markers, hap2_markers; hap1,
hap2) and in the log, whose first line gives k, the marker mode, the threshold and where it came from, both totals and each haplotype's
private k-mers before the solid filter.  A side without a single marker ends the run with exit status 1.  --marker-tables is accepted
and changes nothing: this mode always works that way.  With --markers solid the reads are read twice (once counted, once binned) unless
--child-jf is given.

The reads.  The child's files are read on the host: FASTQ in four-line records or FASTA with one or more sequence lines, line ends LF or
CRLF, plain or .gz.  A read's sequence is its sequence lines without line ends, bytes as they stand (lower case counts as upper case, any
other byte has no k-mer).  The sequences go to the GPU packed back to back in batches of at most --batch-bases bytes (default 256 Mi; a
batch holds at least one read), where KmerTable.read_bins counts per read the windows whose k-mer is a maternal marker (m) and those whose
k-mer is a paternal one (p).  A malformed record ends the run with exit status 1 and a message that names the file and the record.  The
tool's wall time is this reader's; the kernel's share is what JASPER_AMD_TIMING=1 prints.

--reader device parses on the GPU instead: a file's bytes are read as above (open / gzip.open, DEVICE_CHUNK bytes at a time, the unused
tail carried over) and go to HBM as they stand, where KmerTable.read_bins_text finds the lines, verifies the records, packs the sequences
and bins them; only the per-record arrays come back.  Every output file is byte for byte the host reader's.  --batch-bases has no effect
there (a batch is a chunk).  A chunk the GPU calls malformed is parsed once more by the host parser, which words the message.
--write-reads then routes the second pass's bytes by the record starts the first pass has kept (8 bytes a record) instead of parsing
again.  JASPER_TRIOBIN_CHUNK=<bytes> overrides DEVICE_CHUNK.  The default is host.

--gz device (with --reader device) inflates a file whose name ends in .gz on the GPU as well: KmerTable.gz_text opens a session of the
device inflater on the maternal table, and each chunk -- the tail carried over, then DEVICE_CHUNK more inflated bytes -- goes from the
inflater to the parser inside HBM.  The text comes back only with --per-read (the names), and only as far as the records reach; a
malformed chunk comes back whole for the host parser's message.  A file the device inflater refuses (no gzip header, not a regular file)
is read through gzip.open, and JASPER_AMD_TIMING=1 says so.  A CRC or length error, a truncated or a damaged stream end the run with exit
status 1 and a message that names the file.  Plain files go the way they go without the flag.  The default is host.

--route device (with --reader device --write-reads) does the second pass's routing on the GPU: a block's record bounds and bin codes,
computed from the kept starts as before, go to KmerTable.route_text with the block's bytes (a plain file, or a .gz one under --gz host)
or to the session's route (a .gz file under --gz device: the bytes are inflated into HBM and never visit the host unrouted); three
buffers come back and are written to the three files.  The file has changed between the passes when a block comes short, bytes are left
over, or a record's first byte is no longer the records' first byte.  The default is host.

--write-gz (with --write-reads) writes every bin file compressed, as PREFIX.<bin>.<basename>.gz: BGZF (jasper_amd/bgzf.py), a series of
independent gzip members of at most 65280 text bytes each and the 28-byte empty member at the end, which gzip -dc, Python's gzip, bgzip
and this project's readers take -- the files go straight into jasper.sh -r.  A bin without a record gives a file of exactly that empty
member.  Every write cuts its bytes into members on its own and carries no tail to the next, so the member boundaries follow the chunks
(CHUNK, and JASPER_TRIOBIN_CHUNK in the first pass's reader); what is promised is the decompressed content, byte for byte the plain file.
--deflate host (the default) compresses with zlib at level 1 on the host; --deflate device sends each write's bytes through
KmerTable.deflate_bgzf (the GPU compressor: LZ77 and dynamic Huffman codes per member), with any --reader; under --route device the
routed bytes are compressed where they lie in HBM (the _gz route calls) and only the members come back.

--write-jf writes what the polisher reads, not what it would have to count again: PREFIX.<first>.jf and PREFIX.<second>.jf (mat / pat, or
hap1 / hap2), Jellyfish databases of the canonical k-mers of the reads binned <that bin> or unknown -- the sequences as --per-read
measures them -- which go straight into jasper.sh -j:

    python -m jasper_amd.triobin -r 'reads.fq' --hap1 hap1.fa --hap2 hap2.fa --write-jf -o dip
    jasper.sh -a hap1.fa -j dip.hap1.jf ...
    jasper.sh -a hap2.fa -j dip.hap2.jf ...

Counting is additive, so count(own bin + unknown) = count(all reads) - count(other bin), key by key in 64-bit counts.  Once the bins
are known a second pass goes over the inputs with the reader the first pass used (chunks, or the device reader and its gz sessions)
and counts each bin's reads where the batch lies in HBM (KmerTable.count_binned, count_binned_workspace) into T1 (the first bin) and
T2 (the second); the unknown reads, most of a real genome's, are never counted on their own.  The reads' table R is the child's table
of --markers solid, kept open instead of closed (counted, or --child-jf), and otherwise a third sink of the same pass that takes every
read.  Then first.jf = R - T2 (KmerTable.subtract) is written and closed before second.jf = R - T1 is made: the peak is R and one
result.  The header's command line is `count -C -m K -o <file name>` and the read files as given.  A record count that differs from the
first pass's ends the run (FILE changed between the two passes); so does a subtraction that meets a k-mer the reads' table holds less
often than a bin's reads do, which only a --child-jf that is not these reads' database can cause.  Either way no .jf is left.  The log
gets one more line -- per database its bins, reads, bases, distinct k-mers and occurrences -- and JASPER_AMD_TIMING=1 one with the
gather kernels' seconds and bytes, the counting seconds, both subtracts' seconds and counters and the pass's wall time.  Works with or
without --write-reads, in both modes, with every --reader, --gz and --paired combination.

The rule.  A template's m and p are its read's counts; with --paired they are the sums over its two mates.

    m + p < --min-markers (default 1, at least 1)    unknown
    otherwise  m * P_total > p * M_total             mat
    otherwise  m * P_total < p * M_total             pat
    otherwise  (equal)                               unknown

The comparison is exact integer arithmetic: no floating point, and products beyond 2^64 stay exact.

--paired: the files are R1 R2 [R1 R2 ...], record i of each file of a pair is one template.  An odd number of files ends the run before
anything is counted, pair files with different record counts end it when that is found; neither leaves an output file.

The files (each written as .tmp, then renamed; the read files renamed only when the run has succeeded):

    PREFIX.readbins.tsv         #file bin reads bases mat_markers pat_markers: per input file in the order given three rows (mat, pat,
                                unknown), then three rows for file `*` with the sums.  bases = sequence bytes of the bin's reads; the marker
                                columns sum m and p of the bin's reads, each read's own counts, not its template's
    PREFIX.readbins.reads.tsv   with --per-read: #file record name length mat pat bin, one line per read in input order; record is 0-based
                                within its file, name the first token of the header line without @ / >
    PREFIX.<bin>.jf             with --write-jf, for the first two bins: the k-mer database of that bin's and the unknown bin's reads
    PREFIX.<bin>.<basename>     with --write-reads: for each of the three bins and each input file (its base name without a final .gz)
                                that file's records of that bin, byte for byte as they stand in the decompressed input, in input order --
                                the mates of a pair stay in step across R1 and R2, and the three files of an input hold each of its
                                records exactly once.  Written by a second pass over the input with the bins in memory.  Two inputs with
                                one base name end the run before anything is counted.  With --write-gz the names end in .gz and the
                                files are BGZF.

PREFIX defaults to the first read file's name.  The log gives k, both thresholds and where they came from, M_total and P_total, then
reads and bases per bin with their shares.  One GPU; parental tables that do not fit whole on it are an error.
"""
import gzip
import os
import sys
from collections import namedtuple

from . import bgzf, cli, extensions
from .report import write_atomic
from .table import GzText, KmerTable, RoutedText

USAGE = ("Usage: python -m jasper_amd.triobin -r 'child reads...' (--mat 'files' | --mat-jf db.jf) (--pat 'files' | --pat-jf db.jf) [-k 37] [--mat-threshold N] "
         "[--pat-threshold N] [--min-markers N] [--paired] [--per-read] [--write-reads] [--write-jf] [--write-gz (needs --write-reads)] [--deflate host|device (needs --write-gz)] "
         "[--batch-bases N (no effect with --reader device)] [--reader host|device] [--gz host|device (needs --reader device)] "
         "[--route host|device (needs --reader device --write-reads)] [--marker-tables] [-o PREFIX] [--device D]\n"
         "       python -m jasper_amd.triobin -r 'reads...' --hap1 hap1.fa --hap2 hap2.fa [--markers solid|all] [--child-threshold N (with solid)] "
         "[--child-jf db.jf (with solid)] [every other option but the parents']")
BINS = ("mat", "pat", "unknown")
HAP_BINS = ("hap1", "hap2", "unknown")        # assembly mode: the same three roles under the haplotypes' names
MAT, PAT, UNKNOWN = 0, 1, 2
MARKERS = ("solid", "all")
BATCH_BASES_DEFAULT = 256 << 20
BATCH_BASES_MOST = 1 << 40          # (the kernel takes 2^43 text bytes per call)
CHUNK = 16 << 20                    # file bytes parsed at a time
DEVICE_CHUNK = 16 << 20             # ... with --reader device: file bytes uploaded and parsed at a time (JASPER_TRIOBIN_CHUNK overrides it)
DEVICE_CHUNK_MOST = (1 << 30) - 1   # (a chunk and the tail carried into it stay below the kernels' 2^31 text bytes)
READERS = ("host", "device")
BOOL_FLAGS = ("--paired", "--per-read", "--write-reads", "--write-gz", "--marker-tables", "--write-jf")
VALUE_FLAGS = {"-r": "reads", "--reads": "reads", "-k": "k", "--kmer": "k", "-o": "prefix", "--device": "device", "--mat": "mat", "--mat-jf": "mat_jf", "--pat": "pat",
               "--pat-jf": "pat_jf", "--mat-threshold": "mat_threshold", "--pat-threshold": "pat_threshold", "--min-markers": "min_markers", "--batch-bases": "batch_bases",
               "--reader": "reader", "--gz": "gz", "--route": "route", "--deflate": "deflate", "--hap1": "hap1", "--hap2": "hap2", "--markers": "markers",
               "--child-threshold": "child_threshold", "--child-jf": "child_jf"}
PARENT_FLAGS = ("--mat", "--mat-jf", "--pat", "--pat-jf", "--mat-threshold", "--pat-threshold")


class Malformed(Exception):
    """a record that is no FASTQ / FASTA record: (file, 0-based record, what is wrong with it)"""

    def __init__(self, path, record, what):
        Exception.__init__(self, "%s: record %d is malformed: %s" % (path, record, what))


class Inflate(Exception):
    """a .gz file the device inflater cannot read to its end: (file, what the inflater says)"""

    def __init__(self, path, what):
        Exception.__init__(self, "%s: the gzip stream cannot be inflated: %s" % (path, what))


# what a file's reader hands on at a time: `buf` (np.uint8) holds whole records, record i is buf[rec_start[i]:rec_end[i]] and its header
# line ends (without its line end) at head_end[i]; seq = the records' sequences back to back, lens their lengths
Chunk = namedtuple("Chunk", "buf rec_start rec_end head_end seq lens")


def _lines(buf, eof):
    """(starts, ends) of the complete lines of buf: ends[i] is where line i's LF is; at the end of the file a last line without LF counts"""
    import numpy as np
    nl = np.flatnonzero(buf == 10)
    if eof and len(buf) and (len(nl) == 0 or nl[-1] != len(buf) - 1):
        nl = np.append(nl, len(buf))
    ls = np.empty(len(nl), dtype=np.int64)
    if len(nl):
        ls[0] = 0
        ls[1:] = nl[:-1] + 1
    return ls, nl


def _without_cr(buf, ls, le):
    """line ends moved before a CR that stands right before the LF"""
    import numpy as np
    return le - ((le > ls) & (buf[np.maximum(le - 1, 0)] == 13))


def _fastq_chunk(buf, eof, path, nrec, want_seq):
    import numpy as np
    ls, nl = _lines(buf, eof)
    n = len(nl) // 4
    if eof and len(nl) % 4:
        raise Malformed(path, nrec + n, "the file ends inside it")
    if n == 0:
        return 0, None
    ls, nl = ls[:4 * n], nl[:4 * n]
    le = _without_cr(buf, ls, nl)
    bad = (buf[ls[0::4]] != 64) | (buf[ls[2::4]] != 43) | (le[3::4] - ls[3::4] != le[1::4] - ls[1::4])
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        what = "its first line does not begin with @" if buf[ls[4 * i]] != 64 else "its third line does not begin with +" if buf[ls[4 * i + 2]] != 43 else \
            "its quality line is not as long as its sequence"
        raise Malformed(path, nrec + i, what)
    rec_start, rec_end = ls[0::4], np.minimum(nl[3::4] + 1, len(buf))
    used = int(rec_end[-1])
    s, e = ls[1::4], le[1::4]
    seq = None
    if want_seq:
        d = np.zeros(used + 1, dtype=np.int8)
        some = e > s
        d[s[some]] = 1
        d[e[some]] = -1
        seq = buf[:used][np.cumsum(d[:-1], dtype=np.int8).astype(bool)]
    return used, Chunk(buf[:used], rec_start, rec_end, le[0::4], seq, e - s)


def _fasta_chunk(buf, eof, path, nrec, want_seq):
    import numpy as np
    ls, nl = _lines(buf, eof)
    heads = np.flatnonzero(buf[ls] == 62) if len(ls) else np.zeros(0, dtype=np.int64)
    n = len(heads) - (0 if eof else 1)
    if n <= 0:
        return 0, None
    rec_start = ls[heads[:n]]
    rec_end = np.append(ls[heads[1:n]], len(buf) if n == len(heads) else ls[heads[n]])
    used = int(rec_end[-1])
    head_nl = nl[heads[:n]]
    seq_start = np.minimum(head_nl + 1, used)
    keep = np.repeat(np.arange(2 * n) % 2 == 1, np.stack([seq_start - rec_start, rec_end - seq_start], axis=1).ravel())      # header, sequence, header, ...
    view = buf[:used]
    cr = view == 13
    cr[:-1] &= view[1:] == 10
    cr[-1] &= eof and used == len(buf)      # (a CR that ends the file ends its line)
    keep &= (view != 10) & ~cr
    lens = np.add.reduceat(keep, rec_start - rec_start[0], dtype=np.int64)
    return used, Chunk(view, rec_start, rec_end, _without_cr(buf, rec_start, head_nl), view[keep] if want_seq else None, lens)


def chunks(path, want_seq=True):
    """the records of one read file, CHUNK file bytes at a time -> Chunk; raises Malformed"""
    import numpy as np
    parse, carry, nrec = None, b"", 0
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        while True:
            block = f.read(CHUNK)
            eof = not block
            data = carry + block
            if not data:
                return
            if parse is None:
                if data[:1] not in (b"@", b">"):
                    raise Malformed(path, 0, "the file begins with neither @ (FASTQ) nor > (FASTA)")
                parse = _fastq_chunk if data[:1] == b"@" else _fasta_chunk
            used, ch = parse(np.frombuffer(data, dtype=np.uint8), eof, path, nrec, want_seq)
            if ch is not None:
                nrec += len(ch.lens)
                yield ch
            carry = data[used:]
            if eof:
                return


def names_of(ch):
    """the records' names: the first token of the header line without its first byte"""
    out = []
    for a, b in zip(ch.rec_start.tolist(), ch.head_end.tolist()):
        tok = ch.buf[a + 1:b].tobytes().split()
        out.append(tok[0].decode("latin-1") if tok else "")
    return out


def bin_codes(m, p, m_total, p_total, min_markers):
    """the rule, per template -> np.uint8 codes (MAT, PAT, UNKNOWN).  m, p: integer arrays; the products are Python integers"""
    import numpy as np
    out = np.full(len(m), UNKNOWN, dtype=np.uint8)
    m64, p64 = np.asarray(m, dtype=np.uint64), np.asarray(p, dtype=np.uint64)
    if len(out) == 0:
        return out
    if int(m64.max()) * p_total < 1 << 64 and int(p64.max()) * m_total < 1 << 64 and min_markers < 1 << 63:      # both products of every template fit 64 bits: still exact
        a, b = m64 * np.uint64(p_total), p64 * np.uint64(m_total)
        enough = m64 + p64 >= np.uint64(min_markers)
        out[enough & (a > b)] = MAT
        out[enough & (a < b)] = PAT
        return out
    for i in np.flatnonzero((m64 != 0) | (p64 != 0)).tolist():      # (m + p >= min_markers >= 1 needs one of them)
        mi, pi = int(m64[i]), int(p64[i])
        if mi + pi < min_markers:
            continue
        a, b = mi * p_total, pi * m_total
        out[i] = MAT if a > b else PAT if a < b else UNKNOWN
    return out


class _Batcher:
    """reads gathered into batches of at most `room` sequence bytes (at least one read) and counted: count(text, offsets) -> (m, p,
    device seconds).  The counts come back in input order in self.m / self.p (lists of arrays)."""

    def __init__(self, room, count):
        self.room, self.count = room, count
        self.seqs, self.lens, self.bases, self.reads = [], [], 0, 0
        self.m, self.p, self.seconds, self.batches = [], [], 0.0, 0

    def add(self, seq, lens):
        import numpy as np
        c = np.cumsum(lens)
        done, base = 0, 0                               # reads and bytes of this call already placed
        while done < len(lens):
            take = max(0, int(np.searchsorted(c, base + self.room - self.bases, side="right")) - done)
            if take == 0 and self.reads == 0:
                take = 1
            if take == 0:
                self.flush()
                continue
            upto = int(c[done + take - 1])
            self.seqs.append(seq[base:upto])
            self.lens.append(lens[done:done + take])
            self.bases += upto - base
            self.reads += take
            done, base = done + take, upto
            if done < len(lens):
                self.flush()

    def flush(self):
        import numpy as np
        if self.reads == 0:
            return
        offs = np.zeros(self.reads + 1, dtype=np.int64)
        np.cumsum(np.concatenate(self.lens), out=offs[1:])
        m, p, secs = self.count(np.concatenate(self.seqs), offs)
        self.m.append(m)
        self.p.append(p)
        self.seconds += secs
        self.batches += 1
        self.seqs, self.lens, self.bases, self.reads = [], [], 0, 0


def out_basename(path):
    b = os.path.basename(path)
    return b[:-3] if b.endswith(".gz") else b


def _share(a, b):
    return "%.2f %%" % (100.0 * a / b) if b else "NA"


def device_chunk():
    """file bytes per upload of the device reader: DEVICE_CHUNK, or what JASPER_TRIOBIN_CHUNK says"""
    v = os.environ.get("JASPER_TRIOBIN_CHUNK")
    if v is None:
        return DEVICE_CHUNK
    n = int(v) if v.isdigit() else 0
    if not 1 <= n <= DEVICE_CHUNK_MOST:
        cli.error_exit("JASPER_TRIOBIN_CHUNK must be a number of bytes from 1 to %d" % DEVICE_CHUNK_MOST)
    return n


class _HostText:
    """a file read on the host, behind what _DeviceReader uses of a gzip text session: bins(want, fmt) reads up to `want` bytes more into
    ONE buffer for every chunk -- the tail the chunk before left unused at its front, the file read in behind it -- and has
    count_text(buf, eof, fmt) bin them -> table.ReadText (None: no text, or a first byte that is no format's); then n = the text's bytes,
    eof, fmt; text(start, length) = a view of the text, good until the next bins()"""

    def __init__(self, path, count_text):
        self.count_text, self.room, self.n, self.used, self.eof, self.fmt = count_text, bytearray(), 0, 0, False, None
        self.f = gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")
        self.close = self.f.close

    def bins(self, want, fmt):
        have = self.n - self.used
        self.room[:have] = self.room[self.used:self.n]
        if have + want > len(self.room):                # (at first; then for a tail as long as a block: a record longer than that)
            self.room = self.room[:have] + bytearray(want)
        got = self.f.readinto(memoryview(self.room)[have:have + want])
        self.n, self.used, self.eof = have + got, 0, not got
        if self.n and fmt is None:
            self.fmt = {b"@": "fastq", b">": "fasta"}.get(bytes(self.room[:1]))
        if not self.n or self.fmt is None:
            return None
        r = self.count_text(self.text(0, self.n), self.eof, self.fmt)
        self.used = r.used
        return r

    def text(self, start, length):
        import numpy as np
        return np.frombuffer(self.room, dtype=np.uint8, count=length, offset=start)


class _DeviceReader:
    """--reader device: a file's bytes go to the GPU as they stand, count_text(buf, eof, fmt) -> table.ReadText parses, packs and counts
    them there.  chunks(path) yields what the host reader's chunks() yields, without the sequences; the counts come back in input order in
    self.m / self.p as _Batcher has them.  With keep_starts, self.starts[path] = (the records' first byte, their absolute starts in the
    decompressed file, its length): what the second pass of --write-reads routes by.
    --gz device: gz_open(path) -> a gzip text session (table.GzText with the parents bound: bins(want, fmt)) or an exception for a file
    the device inflater refuses; a .gz file's chunks then come from the session instead of a _HostText, and the text, which stays in HBM,
    is fetched only for the names (per_read) and for a malformed chunk."""

    def __init__(self, count_text, keep_starts, gz_open=None, per_read=False):
        self.count_text, self.keep_starts, self.gz_open, self.per_read = count_text, keep_starts, gz_open, per_read
        self.m, self.p, self.seconds, self.starts = [], [], 0.0, {}
        self.inflate_seconds, self.gz_stats = 0.0, []       # the sessions' summed pull seconds (HIP events around each pull), (path, stats) per session

    def chunks(self, path):
        import numpy as np
        sess = open_session(self.gz_open, path)
        src = sess if sess is not None else _HostText(path, self.count_text)
        want = device_chunk()
        fmt, first, nrec, base, have, starts = None, b"", 0, 0, 0, []
        try:
            while True:
                try:
                    r = src.bins(want, fmt)
                except RuntimeError as e:
                    if sess is None:
                        raise
                    raise Inflate(path, str(e))
                n, eof = src.n, src.eof
                if not n:
                    break
                if src.fmt is None:                     # (the host's first byte, or the session's no_format)
                    raise Malformed(path, 0, "the file begins with neither @ (FASTQ) nor > (FASTA)")
                if fmt is None:
                    fmt = src.fmt
                    first = b"@" if fmt == "fastq" else b">"
                if r.malformed:                         # the host parser words the message: the same (buf, eof) raises there
                    (_fastq_chunk if fmt == "fastq" else _fasta_chunk)(src.text(0, n), eof, path, nrec, False)
                    raise RuntimeError("%s: the device reader calls record %d malformed and the host parser does not" % (path, nrec + r.bad_record))
                self.seconds += r.seconds
                if r.n_records:
                    nrec += r.n_records
                    self.m.append(r.mat)
                    self.p.append(r.pat)
                    if self.keep_starts:
                        starts.append(r.rec_start[:-1] + base)
                    # (the host's text is a view of its buffer: looked at before the buffer is used again)
                    yield Chunk(src.text(0, r.used) if sess is None or self.per_read else None, r.rec_start[:-1], r.rec_start[1:], r.head_end, None, r.lens)
                have = n - r.used
                base += r.used
                if eof:
                    break
        finally:
            if sess is not None:
                self.inflate_seconds += sess.inflate_seconds
                self.gz_stats.append((path, sess.stats()))
            src.close()
        if self.keep_starts:
            self.starts[path] = (first, np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64), base + have)


def open_session(gz_open, path):
    """--gz device: the gzip text session of a .gz file, or None -- no gz_open, a plain file, or a file the device inflater refuses, which
    is then read through gzip.open (JASPER_AMD_TIMING=1 says so)"""
    if gz_open is None or not path.endswith(".gz"):
        return None
    try:
        return gz_open(path)
    except RuntimeError as e:
        extensions.device_line("[triobin] gz %s: not for the device inflater, read through gzip.open (%s)" % (path, e))
        return None


def block_segments(starts, at, end):
    """the second pass's block [at, end) of a file whose records begin at `starts` (starts[0] == 0, increasing) -> (i0, i1, bounds,
    check_from): records i0 .. i1 - 1 have bytes in the block, bounds[i1 - i0 + 1] cut the block into their parts (bounds[0] = 0,
    bounds[-1] = end - at), and check_from is 1 when the first part is the clipped rest of a record, which has no first byte to check"""
    import numpy as np
    i0 = int(np.searchsorted(starts, at, side="right")) - 1       # the record the block's first byte lies in
    i1 = int(np.searchsorted(starts, end, side="left"))
    bounds = np.empty(i1 - i0 + 1, dtype=np.int64)
    bounds[0] = 0
    bounds[1:-1] = starts[i0 + 1:i1] - at
    bounds[-1] = end - at
    return i0, i1, bounds, 0 if starts[i0] == at else 1


class _Deflater:
    """--deflate device: deflate(np.uint8 array) -> (its BGZF members, the compressor's counters, device seconds), KmerTable.deflate_bgzf.
    An instance is what a bin file's writer compresses with, and it keeps the sums JASPER_AMD_TIMING=1 prints; note() adds what a _gz
    route call has compressed"""

    def __init__(self, deflate):
        self.deflate, self.seconds, self.counters = deflate, 0.0, dict.fromkeys(("stored", "literal_only", "lz"), 0)

    def note(self, counters, seconds):
        self.seconds += seconds
        for key in self.counters:
            self.counters[key] += counters[key]

    def __call__(self, arr):
        out, counters, seconds = self.deflate(arr)
        self.note(counters, seconds)
        return out


class _BinFiles:
    """the three bin files of one input, as .tmp: plain, or BGZF with --write-gz (deflater: None for the host's zlib, a _Deflater for the
    GPU).  write(b, arr) takes bytes of bin b; write_routed(r) what a route call returns -- bytes, or with gz members and their raw sizes"""

    def __init__(self, prefix, path, made, write_gz=False, deflater=None, sums=None, names=BINS):
        outs = ["%s.%s.%s%s" % (prefix, b, out_basename(path), ".gz" if write_gz else "") for b in names]
        made += outs
        self.sums, self.w = sums, []
        try:
            for fn in outs:
                f = open(fn + ".tmp", "wb")
                self.w.append(bgzf.BgzfWriter(f, deflater or bgzf.compress) if write_gz else bgzf.PlainWriter(f))
        except BaseException:
            self.close()
            raise

    def write(self, b, arr):
        self.w[b].write(arr)

    def write_routed(self, r):
        for b in range(3):
            if getattr(r, "raw_bytes", None) is None:
                self.w[b].write(r.out[b])
            else:
                self.w[b].write_members(r.out[b], r.raw_bytes[b])

    def close(self):
        """every file is closed, whatever closing one of them raises (the end marker may not fit the disk): the first error leaves"""
        writers, self.w, error = self.w, [], None
        for w in writers:
            try:
                w.close()
            except BaseException as e:      # noqa: B902  (re-raised below)
                error = error or e
                try:
                    w.f.close()
                except OSError:
                    pass
            if self.sums is not None:
                self.sums["deflate_raw"] = self.sums.get("deflate_raw", 0) + w.raw
                self.sums["deflate_written"] = self.sums.get("deflate_written", 0) + w.written
        if error is not None:
            raise error


def bin_files(paths, prefix, count, m_total, p_total, min_markers=1, paired=False, per_read=False, write_reads=False, batch_bases=BATCH_BASES_DEFAULT, reader="host",
              count_text=None, gz_open=None, route_text=None, timings=None, write_gz=False, deflate=None, names=BINS, write_jf=None):
    """everything after the parents: read, count (count(text, offsets) -> (m, p, seconds)), bin, write.  Errors leave through
    cli.error_exit before any output file exists; -> (reads, bases) per bin and the counter's summed seconds.  reader "device": the files'
    bytes are parsed and counted by count_text (_DeviceReader) and `count` is not called.  gz_open: --gz device (_DeviceReader);
    route_text: --route device, route_text(buf, bounds, bins, first, check_from, out) -> table.RoutedText.  timings (a dict) gets what
    JASPER_AMD_TIMING=1 prints of the two.  write_gz: the bin files are BGZF; deflate (--deflate device): deflate(array) -> (members,
    counters, seconds) compresses them, and with route_text the route calls are made with gz=True and return members.  names: what the
    three bins are called in the file names, in both tables and, the first two, in the marker and per-read columns (HAP_BINS in assembly
    mode).  write_jf (--write-jf): write_jf(bins, nrec, made) is called once the bins are known, writes its databases as .tmp and adds
    their names to `made`, the list of what is renamed when the run has succeeded (a _WriteJf)"""
    import numpy as np
    bat = _Batcher(batch_bases, count)
    deflater = _Deflater(deflate) if write_gz and deflate is not None else None
    dev = _DeviceReader(count_text, write_reads, gz_open, per_read) if reader == "device" else None
    timings = {} if timings is None else timings
    nrec, lens, rnames = [], [], []
    try:
        for fi, path in enumerate(paths):
            fl, fn = [], []
            for ch in (dev.chunks(path) if dev else chunks(path)):
                fl.append(ch.lens)
                if per_read:
                    fn += names_of(ch)
                if dev:
                    continue
                bat.add(ch.seq, ch.lens)
            lens.append(np.concatenate(fl) if fl else np.zeros(0, dtype=np.int64))
            nrec.append(len(lens[-1]))
            rnames.append(fn)
            if paired and fi % 2 == 1 and nrec[fi] != nrec[fi - 1]:
                cli.error_exit("--paired: %s has %d records and %s has %d; the files of a pair must hold the same templates" % (paths[fi - 1], nrec[fi - 1], path, nrec[fi]))
        bat.flush()
    except (Malformed, Inflate) as e:
        cli.error_exit(str(e))
    finally:
        if dev:
            timings.update(inflate_seconds=dev.inflate_seconds, gz_stats=dev.gz_stats)
    if dev:
        bat.m, bat.p, bat.seconds = dev.m, dev.p, dev.seconds
    cuts = np.cumsum(nrec)[:-1]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)      # noqa: E731
    ms, ps = np.split(cat(bat.m), cuts), np.split(cat(bat.p), cuts)
    bins = []
    for fi in range(len(paths)):
        if paired and fi % 2 == 1:
            bins.append(bins[-1])
        elif paired:
            bins.append(bin_codes(ms[fi].astype(np.uint64) + ms[fi + 1], ps[fi].astype(np.uint64) + ps[fi + 1], m_total, p_total, min_markers))
        else:
            bins.append(bin_codes(ms[fi], ps[fi], m_total, p_total, min_markers))
    # the table
    text = "#file\tbin\treads\tbases\t%s_markers\t%s_markers\n" % names[:2]
    total = np.zeros((3, 4), dtype=object)
    for fi, path in enumerate(paths):
        for b in range(3):
            sel = bins[fi] == b
            row = [int(sel.sum()), int(lens[fi][sel].sum()), int(ms[fi][sel].sum(dtype=np.uint64)), int(ps[fi][sel].sum(dtype=np.uint64))]
            total[b] += row
            text += "%s\t%s\t%d\t%d\t%d\t%d\n" % (path, names[b], row[0], row[1], row[2], row[3])
    text += "".join("*\t%s\t%d\t%d\t%d\t%d\n" % ((names[b],) + tuple(int(v) for v in total[b])) for b in range(3))
    made = []
    opened = lambda path: _BinFiles(prefix, path, made, write_gz, deflater, timings if write_gz else None, names)      # noqa: E731
    try:
        if write_reads and dev:
            _write_reads_by_starts(paths, opened, bins, dev.starts, route_text, gz_open, timings, deflater)
        elif write_reads:
            _write_reads(paths, opened, bins, nrec)
        if deflater is not None:
            timings.update(deflate_seconds=deflater.seconds, deflate_blocks=deflater.counters)
        if write_jf is not None:
            write_jf(bins, nrec, made)
        write_atomic(prefix + ".readbins.tsv", text)
        if per_read:
            with open(prefix + ".readbins.reads.tsv.tmp", "w") as f:
                made.append(prefix + ".readbins.reads.tsv")
                f.write("#file\trecord\tname\tlength\t%s\t%s\tbin\n" % names[:2])
                for fi, path in enumerate(paths):
                    f.writelines("%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % (path, i, rnames[fi][i], lens[fi][i], ms[fi][i], ps[fi][i], names[bins[fi][i]]) for i in range(nrec[fi]))
        for fn in made:
            os.replace(fn + ".tmp", fn)
        made = []
    finally:
        for fn in made:                                 # a run that has not succeeded leaves no read file behind
            if os.path.exists(fn + ".tmp"):
                os.remove(fn + ".tmp")
    return [(int(total[b][0]), int(total[b][1])) for b in range(3)], bat.seconds


def _write_reads(paths, opened, bins, nrec):
    """the second pass: every input's records into its three .tmp files (opened(path) -> _BinFiles, which notes the names they are to have)"""
    import numpy as np
    for fi, path in enumerate(paths):
        files = opened(path)
        try:
            at = 0
            try:
                for ch in chunks(path, want_seq=False):
                    n = len(ch.lens)
                    if at + n > nrec[fi]:
                        break
                    size = ch.rec_end - ch.rec_start
                    for b in range(3):
                        files.write(b, ch.buf[np.repeat(bins[fi][at:at + n] == b, size)])
                    at += n
            except Malformed:
                at = -1
            if at != nrec[fi]:
                cli.error_exit("--write-reads: %s changed between the two passes" % path)
        finally:
            files.close()


def _route_by_masks(buf, bounds, codes, first, check_from, out):
    """what route_text computes, on the host: three boolean masks, and the count of starts that do not hold the records' first byte"""
    import numpy as np
    size = np.diff(bounds)
    return RoutedText([buf[np.repeat(codes == b, size)] for b in range(3)], int((buf[bounds[check_from:-1]] != first[0]).sum()), 0.0)


class _FileBlocks:
    """a file read on the host, behind what the second pass uses of a gzip text session: route(want, bounds, codes, first, check_from, out)
    reads the next `want` bytes (`got` of them) and, when they are the bytes the bounds were made for (`routed`), has route_text route
    them -- KmerTable.route_text (--route device) or _route_by_masks"""

    def __init__(self, path, route_text):
        self.route_text = route_text
        self.f = gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")
        self.close = self.f.close

    def route(self, want, bounds, codes, first, check_from, out, **gz):
        import numpy as np
        buf = np.frombuffer(self.f.read(want), dtype=np.uint8)
        if not len(buf) or len(buf) != bounds[-1]:
            return RoutedText(None, 0, 0.0, len(buf), False)
        r = self.route_text(buf, bounds, codes, first, check_from, out, **gz)
        r.got, r.routed = len(buf), True
        return r


def _write_reads_by_starts(paths, opened, bins, kept, route_text=None, gz_open=None, timings=None, deflater=None):
    """the second pass of the device reader: nothing is parsed again, a block's bytes are routed by the record starts the first pass has
    kept.  The file has changed when its decompressed length differs or a remembered start does not hold the records' first byte.
    route_text (--route device) routes a block on the GPU instead of with three boolean masks; gz_open then inflates a .gz file there too;
    deflater (--write-gz --deflate device) then has the route calls compress the three outputs there as well (gz=True)"""
    import numpy as np
    import time
    t0 = time.perf_counter()
    route_seconds, inflate_seconds, gz_stats = 0.0, 0.0, []
    gz = {"gz": True} if route_text and deflater is not None else {}
    room = CHUNK + (31 * (-(-CHUNK // bgzf.BLOCK)) if gz else 0)        # (a member adds at most 31 bytes to its text)
    out = [np.empty(room, dtype=np.uint8) for _ in range(3)] if route_text else None
    for fi, path in enumerate(paths):
        files = opened(path)
        first, starts, length = kept[path]
        sess = open_session(gz_open, path) if route_text else None
        src = sess
        try:
            if sess is None:
                src = _FileBlocks(path, route_text or _route_by_masks)
            at = 0
            try:
                while 0 <= at < length:
                    end = min(at + CHUNK, length)
                    i0, i1, bounds, check_from = block_segments(starts, at, end)
                    r = src.route(end - at, bounds, bins[fi][i0:i1], first, check_from, out, **gz)
                    route_seconds += r.seconds
                    if not r.routed or r.mismatches:    # (a block that came short; a start that does not hold the records' first byte)
                        at = -1
                        break
                    if gz:
                        deflater.note(r.deflate, r.deflate_seconds)
                    files.write_routed(r)
                    at = end
                if at == length and src.route(1, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint8), first, 0, out).got:      # (bytes are left over)
                    at = -1
            except RuntimeError as e:
                if sess is None:
                    raise
                cli.error_exit(str(Inflate(path, str(e))))
            if at != length:
                cli.error_exit("--write-reads: %s changed between the two passes" % path)
        finally:
            if sess is not None:
                inflate_seconds += sess.inflate_seconds
                gz_stats.append((path, sess.stats()))
            if src is not None:
                src.close()
            files.close()
    if timings is not None:
        timings.update(route_seconds=route_seconds, route_inflate_seconds=inflate_seconds, route_gz_stats=gz_stats, second_pass_wall=time.perf_counter() - t0)


class _WriteJf:
    """--write-jf: once the bins are known, a second pass over the inputs counts the reads of the first bin into T1 and those of the
    second into T2 (and, where the reads' table R is not at hand, all of them into R), then first.jf = R - T2 is written and closed
    and second.jf = R - T1 after it.  tables: the run's _Tables (the device reader parses and packs on its maternal table, whose
    workspace the counting reads); reads_table: R kept from the markers (assembly mode, --markers solid), or None.  An instance is
    bin_files' write_jf; afterwards `databases` holds per file (name, bins, distinct, occurrences) and `timing` what
    JASPER_AMD_TIMING=1 prints"""

    def __init__(self, tables, reads_table, k, device, prefix, names, paths, reader, gz_open):
        self.tables, self.reads_table, self.k, self.device, self.prefix, self.names = tables, reads_table, k, device, prefix, names
        self.paths, self.reader, self.gz_open = paths, reader, gz_open
        self.databases, self.timing = [], {}

    def count_pass(self, bins, nrec, sinks):
        """every input once more, with the first pass's reader: a chunk's sequences and its reads' codes go to the sinks -> the sums of
        the sinks' stats.  A record count that is not the first pass's ends the run"""
        import numpy as np
        sums = [dict(reads=0, bases=0, occurrences=0, gather_seconds=0.0, count_seconds=0.0) for _ in sinks]
        t = self.tables
        dev = _DeviceReader(t.count_text, False, self.gz_open, False) if self.reader == "device" else None
        for fi, path in enumerate(self.paths):
            at = 0
            try:
                for ch in (dev.chunks(path) if dev else chunks(path)):
                    n = len(ch.lens)
                    if at + n > nrec[fi]:
                        at = -1
                        break
                    codes = bins[fi][at:at + n]
                    if dev:                             # (the chunk's packed sequences are what the maternal table's workspace holds now)
                        stats = KmerTable.count_binned_workspace(t.mat, t.pat, n, codes, sinks)
                    else:
                        offs = np.zeros(n + 1, dtype=np.int64)
                        np.cumsum(ch.lens, out=offs[1:])
                        stats = KmerTable.count_binned((ch.seq, offs), codes, sinks)
                    for total, st in zip(sums, stats):
                        for key in total:
                            total[key] += st[key]
                    at += n
            except (Malformed, Inflate):
                at = -1
            if at != nrec[fi]:
                cli.error_exit("--write-jf: %s changed between the two passes" % path)
        return sums

    def __call__(self, bins, nrec, made):
        import time
        t0 = time.perf_counter()
        opened = []
        table = lambda: opened.append(KmerTable(self.k, min_slots=1 << 20, device=self.device)) or opened[-1]      # noqa: E731
        try:
            first, second = table(), table()
            sinks = [(first, (MAT,)), (second, (PAT,))]
            reads = self.reads_table
            if reads is None:
                reads = table()
                sinks.append((reads, (MAT, PAT, UNKNOWN)))
            sums = self.count_pass(bins, nrec, sinks)
            subtracts = []
            for own, minus in ((MAT, second), (PAT, first)):
                fn = "%s.%s.jf" % (self.prefix, self.names[own])
                dst, st = KmerTable.subtract(reads, minus)
                try:
                    subtracts.append(st)
                    if st["underflow"] or st["missing"]:
                        cli.error_exit("--write-jf: the reads' k-mer table holds %d k-mers of the %s reads less often than those reads do and lacks %d of them: "
                                       "--child-jf is not the database of these reads" % (st["underflow"], self.names[1 - own], st["missing"]))
                    made.append(fn)
                    dst.write_jf(fn + ".tmp", ["count", "-C", "-m", str(self.k), "-o", fn] + list(self.paths))
                    info = dst.info()
                    self.databases.append((fn, (self.names[own], self.names[UNKNOWN]), info["distinct"], info["occurrences"]))
                finally:
                    dst.close()
        finally:
            for t in opened:
                t.close()
        self.timing = dict(sums=sums, subtracts=subtracts, wall=time.perf_counter() - t0)

    def log(self, per_bin):
        """the log's line after `Read bins:`, and JASPER_AMD_TIMING=1's"""
        cli.log("K-mer databases: " + "; ".join("%s of the %s and %s reads: %d reads, %d bases, %d distinct k-mers, %d occurrences" % (
            fn, b[0], b[1], per_bin[i][0] + per_bin[UNKNOWN][0], per_bin[i][1] + per_bin[UNKNOWN][1], distinct, occ) for i, (fn, b, distinct, occ) in enumerate(self.databases)))
        if self.timing:
            sums, subs = self.timing["sums"], self.timing["subtracts"]
            extensions.device_line("[triobin] write-jf: gather kernels device seconds %.6f for %d bytes; counting seconds %.6f; subtract device seconds %s; pass wall seconds %.6f" % (
                sum(s["gather_seconds"] for s in sums), sum(s["bases"] + s["reads"] for s in sums), sum(s["count_seconds"] for s in sums),
                "; ".join("%s %.6f (swept %d, matched %d, dropped %d, underflow %d, kept %d)" % (
                    self.names[i], st["seconds"], st["swept"], st["matched"], st["dropped"], st["underflow"], st["kept"]) for i, st in enumerate(subs)),
                self.timing["wall"]))


def check_write_jf(a, hap, prefix, names):
    """--write-jf: refused before anything is opened -- a database it would write is the one --child-jf reads"""
    if not a["write_jf"]:
        return
    child = hap.get("child_jf")
    for fn in ("%s.%s.jf" % (prefix, b) for b in names[:2]):
        if child is not None and os.path.abspath(fn) == os.path.abspath(child):
            cli.error_exit("--write-jf: %s would be written over the --child-jf database; give another prefix with -o" % fn)


def parse_args(argv):
    o = dict.fromkeys(set(VALUE_FLAGS.values()))
    o.update(k="37", device="0", paired=False, per_read=False, write_reads=False, write_gz=False, marker_tables=False, write_jf=False)
    i = 0
    while i < len(argv):
        key = argv[i]
        if key in ("-h", "--help"):
            print(USAGE)
            sys.exit(0)
        if key in BOOL_FLAGS:
            o[extensions.flag_attr(key)] = True
            i += 1
            continue
        if key not in VALUE_FLAGS or i + 1 >= len(argv):
            print("Unknown option %s" % key)
            sys.exit(1)
        o[VALUE_FLAGS[key]] = argv[i + 1]
        i += 2
    return o


def check_haps(a):
    """assembly mode's flags, refused before anything is opened -> None (trio mode) or dict(hap1, hap2, markers, thre_child (None: from the
    histogram; not used with markers all), child_jf)"""
    on = a["hap1"] is not None or a["hap2"] is not None
    if not on:
        for flag in ("--markers", "--child-threshold", "--child-jf"):
            if a[VALUE_FLAGS[flag]] is not None:
                cli.error_exit("%s is an option of binning by two haplotype assemblies: give --hap1 and --hap2 as well" % flag)
        return None
    for flag, other in (("--hap1", "--hap2"), ("--hap2", "--hap1")):
        if a[VALUE_FLAGS[other]] is None:
            cli.error_exit("%s needs %s: the reads are binned by the two haplotypes of one assembly" % (flag, other))
    for flag in PARENT_FLAGS:
        if a[VALUE_FLAGS[flag]] is not None:
            cli.error_exit("%s cannot be given with --hap1 / --hap2: the markers come either from the parents' reads or from the two haplotype assemblies" % flag)
    for flag in ("--hap1", "--hap2"):
        if not cli._nonempty(a[VALUE_FLAGS[flag]]):
            cli.error_exit("%s: %s does not exist or is empty. Please supply that haplotype's fasta file." % (flag, a[VALUE_FLAGS[flag]]))
    if os.path.samefile(a["hap1"], a["hap2"]):
        cli.error_exit("--hap2: %s is the --hap1 assembly itself; give the OTHER haplotype's fasta file" % a["hap2"])
    markers = a["markers"] if a["markers"] is not None else "solid"
    if markers not in MARKERS:
        cli.error_exit("--markers takes solid or all; %s was given" % markers)
    if markers == "all":
        for flag in ("--child-jf", "--child-threshold"):
            if a[VALUE_FLAGS[flag]] is not None:
                cli.error_exit("%s has no use with --markers all: only --markers solid looks at the child's k-mers" % flag)
    thre = extensions._range_flag("--child-threshold", a["child_threshold"], None, 1, 0xFFFFFFFF)
    if a["child_jf"] is not None and not cli._nonempty(a["child_jf"]):
        cli.error_exit("--child-jf: %s does not exist or is empty" % a["child_jf"])
    return dict(hap1=a["hap1"], hap2=a["hap2"], markers=markers, thre_child=thre, child_jf=a["child_jf"])


def check_flags(a):
    """everything that can be refused before a parent is opened -> (read files, k, device, the parents' flags (assembly mode: check_haps'
    dict), min_markers, batch_bases)"""
    if a["reads"] is None:
        cli.error_exit("No reads given. Please supply the child's read files with -r, separated by space and wrapped in one pair of quotation marks.")
    opts = cli.Options()
    opts.reads = a["reads"]
    reads = cli._reads(opts)
    if not reads:
        cli.error_exit("No reads given. Please supply the child's read files with -r, separated by space and wrapped in one pair of quotation marks.")
    k = extensions._range_flag("-k", a["k"], 37, 1, 64)
    device = extensions._range_flag("--device", a["device"], 0, 0, 1023)
    min_markers = extensions._range_flag("--min-markers", a["min_markers"], 1, 1, 1 << 33)
    batch_bases = extensions._range_flag("--batch-bases", a["batch_bases"], BATCH_BASES_DEFAULT, 1, BATCH_BASES_MOST)
    hap = check_haps(a)
    if hap is not None:
        if hap["child_jf"] is not None:                 # (a database's header decides k)
            k = extensions.jf_k(hap["child_jf"])
            if k is None:
                cli.error_exit("--child-jf: " + cli._jf_failed(hap["child_jf"]))
    else:
        o = type("TriobinOptions", (), dict(a, hapmers=True, phase_short_range=None, phase_max_switches=None))
        first_jf = a["mat_jf"] if a["mat_jf"] is not None else a["pat_jf"]
        hap = extensions.hapmer_flags(o, k, first_jf)       # (a database's header decides k; both parents must have it)
        if first_jf is not None:
            k = extensions.jf_k(first_jf)
    if a["paired"] and len(reads) % 2:
        cli.error_exit("--paired takes the read files as R1 R2 [R1 R2 ...]; %d files were given" % len(reads))
    if a["write_reads"]:
        seen = {}
        for fn in reads:
            if out_basename(fn) in seen:
                cli.error_exit("--write-reads: %s and %s would be written to the same files; give inputs with different base names" % (seen[out_basename(fn)], fn))
            seen[out_basename(fn)] = fn
    return reads, k, device, hap, min_markers, batch_bases


def _host_or_device(a, flag):
    """the value of a flag that takes host or device: host when it is not given"""
    v = a[VALUE_FLAGS[flag]] if a[VALUE_FLAGS[flag]] is not None else "host"
    if v not in READERS:
        cli.error_exit("%s takes host or device; %s was given" % (flag, v))
    return v


def check_reader(a):
    """--reader, and with device the chunk size: refused before a parent is opened"""
    reader = _host_or_device(a, "--reader")
    if reader == "device":
        device_chunk()
    return reader


def check_gz_route(a, reader):
    """--gz and --route: refused before a parent is opened -> (gz, route)"""
    gz, route = _host_or_device(a, "--gz"), _host_or_device(a, "--route")
    if gz == "device" and reader != "device":
        cli.error_exit("--gz device needs --reader device: the inflated text goes to the device reader inside the GPU's memory")
    if route == "device" and not (reader == "device" and a["write_reads"]):
        cli.error_exit("--route device needs --reader device --write-reads: it routes the second pass by the record starts the device reader keeps")
    return gz, route


def check_write_gz(a):
    """--write-gz and --deflate: refused before a parent is opened -> (write_gz, deflate)"""
    deflate = _host_or_device(a, "--deflate")
    if a["write_gz"] and not a["write_reads"]:
        cli.error_exit("--write-gz needs --write-reads: it is the bin files that are written compressed")
    if a["deflate"] is not None and not a["write_gz"]:
        cli.error_exit("--deflate %s needs --write-gz: it says where the bin files are compressed" % deflate)
    return a["write_gz"], deflate


def check_totals(m_total, p_total):
    """a parent without a single hap-mer ends the run: the rule has nothing to weigh"""
    if m_total == 0 or p_total == 0:
        cli.error_exit("The %s no hap-mers at these thresholds: nothing tells the parents' reads apart." % (
            "parents have" if m_total == p_total else "mother has" if m_total == 0 else "father has"))


class _Tables:
    """the two tables and their thresholds, bound into what bin_files calls: count, count_text, gz_open, route_text, deflate.  Every
    chunk's ReadText passes note(): index_seconds and text_bytes are the run's sums of index + pack seconds and of the bytes records cover"""

    def __init__(self, mat, pat, thre_mat, thre_pat):
        self.mat, self.pat, self.thre_mat, self.thre_pat = mat, pat, thre_mat, thre_pat
        self.index_seconds, self.text_bytes = 0.0, 0

    def note(self, r):
        self.index_seconds += r.index_seconds
        self.text_bytes += r.used
        return r

    def count(self, text, offs):
        r = KmerTable.read_bins(self.mat, self.pat, (text, offs), self.thre_mat, self.thre_pat)
        return r.mat, r.pat, r.seconds

    def count_text(self, buf, eof, fmt):
        return self.note(KmerTable.read_bins_text(self.mat, self.pat, buf, eof, fmt, self.thre_mat, self.thre_pat))

    def gz_open(self, path):
        return _Session(self, path)

    def route_text(self, buf, bounds, codes, first, check_from, out, gz=False):
        return self.mat.route_text(buf, bounds, codes, first, check_from, out, gz=gz)

    def deflate(self, arr):
        return self.mat.deflate_bgzf(arr)


class _Session(GzText):
    """a table.GzText on the maternal table with the father's table and the thresholds bound: bins(want, fmt), what _DeviceReader drives"""

    def __init__(self, tables, path):
        GzText.__init__(self, tables.mat, path)
        self.tables = tables

    def bins(self, want, fmt):
        t = self.tables
        return t.note(GzText.bins(self, t.pat, want, fmt, t.thre_mat, t.thre_pat))


def timing_lines(t, gz, route, deflate=None):
    """JASPER_AMD_TIMING=1: what --gz device, --route device and --write-gz add"""
    stat = lambda st: " ".join("%s=%d" % kv for kv in st.items())      # noqa: E731
    if gz == "device":
        extensions.device_line("[triobin] gz inflate seconds by events: %.6f (first pass; the inflater's kernels and copies and the host's stitching between them)" % t.get("inflate_seconds", 0.0))
        for path, st in t.get("gz_stats", []):
            extensions.device_line("[triobin] gz stats %s: %s" % (path, stat(st)))
    if "second_pass_wall" in t:
        extensions.device_line("[triobin] second pass wall seconds: %.6f" % t["second_pass_wall"])
    if route == "device" and "route_seconds" in t:
        extensions.device_line("[triobin] route kernels device seconds: %.6f; gz inflate seconds by events: %.6f (second pass)" % (t["route_seconds"], t["route_inflate_seconds"]))
        for path, st in t["route_gz_stats"]:
            extensions.device_line("[triobin] gz stats %s (second pass): %s" % (path, stat(st)))
    if deflate is not None and "deflate_raw" in t:
        c = t.get("deflate_blocks", {})
        extensions.device_line("[triobin] deflate %s: kernels device seconds %s; %d raw bytes, %d compressed bytes; blocks stored %s, literal-only %s, LZ %s" % (
            deflate, "%.6f" % t["deflate_seconds"] if "deflate_seconds" in t else "NA", t["deflate_raw"], t["deflate_written"], c.get("stored", "NA"),
            c.get("literal_only", "NA"), c.get("lz", "NA")))


def haps_totals_check(m_total, p_total):
    """check_totals for two haplotype assemblies: a side without a single marker ends the run"""
    if m_total == 0 or p_total == 0:
        cli.error_exit("%s no marker k-mers: nothing tells the two haplotypes' reads apart." % (
            "The haplotypes have" if m_total == p_total else "hap1 has" if m_total == 0 else "hap2 has"))


def marker_tables(first, second, solid, thre_first, thre_second, thre_solid):
    """the two marker sets as tables (KmerTable.select): the keys of `first` (count >= thre_first) that `second` does not hold and,
    with `solid`, that it holds at least thre_solid times, and the mirror -> (M', P', the two selects' stats); the caller closes them"""
    from .table import KmerTable
    m, sm = KmerTable.select(first, second, solid, thre_first, thre_solid)
    try:
        p, sp = KmerTable.select(second, first, solid, thre_second, thre_solid)
    except BaseException:
        m.close()
        raise
    return m, p, sm, sp


def select_line(names, stats):
    """JASPER_AMD_TIMING=1: both selects' device seconds and their four counters"""
    extensions.device_line("[triobin] select device seconds: " + "; ".join(
        "%s %.6f (candidates %d, in_absent %d, not_solid %d, selected %d)" % (n, st["seconds"], st["candidates"], st["in_absent"], st["not_solid"], st["selected"])
        for n, st in zip(names, stats)))


def child_table(hap, reads, k, device):
    """--markers solid: the child's reads counted into a table (as kmerqc counts -r), or --child-jf loaded, and the threshold --
    --child-threshold, or what the solid-k-mer rule derives from the histogram -> (KmerTable, threshold, where it came from)"""
    from . import polisher
    from .table import KmerTable
    try:
        if hap["child_jf"] is not None:
            t = KmerTable.from_jf(hap["child_jf"], device=device)
        else:
            size = sum(os.stat(fn).st_size for fn in reads) // 10
            t = KmerTable(k, min_slots=max(1 << 20, int(1.25 * size)), device=device)
            try:
                t.count_files(reads)
            except BaseException:
                t.close()
                raise
    except Exception as e:      # noqa: BLE001
        cli.error_exit("--markers solid: the child's table could not be made on GPU %d: %s" % (device, e))
    if hap["thre_child"] is not None:
        return t, hap["thre_child"], "given"
    txt, status = polisher.threshold_from_histo_rows(t.histo_rows())
    if status != 0 or not txt.split() or int(txt.split()[0]) < 1:
        t.close()
        cli.error_exit("The child's reads' k-mer histogram gives no threshold. Please give one with --child-threshold.")
    return t, int(txt.split()[0]), "from the histogram"


def open_haps(hap, reads, k, device, keep_child=False):
    """assembly mode: both assemblies counted (as kmerqc counts -a and --alt), with --markers solid the child's table beside them, the
    two selects, the three source tables closed -> (M', P', M_total, P_total, None); the caller closes M' and P'.  keep_child
    (--write-jf): the child's table of --markers solid is not closed but returned in the None's place, and is the caller's to close.
    Writes the mode's log line."""
    tables, child, done = [], None, False
    try:
        for fn in (hap["hap1"], hap["hap2"]):
            tables.append(extensions.contigs_table(k, device, extensions.Text(fn).contigs))
        thre, origin = 1, None
        if hap["markers"] == "solid":
            child, thre, origin = child_table(hap, reads, k, device)
            tables.append(child)
        m, p, sm, sp = marker_tables(tables[0], tables[1], tables[2] if len(tables) > 2 else None, 1, 1, thre)
        done = True
    finally:
        for t in tables:
            if not (done and keep_child and t is child):
                t.close()
    if not keep_child:
        child = None
    try:                                                # (the marker tables, and a kept child's, are this function's until it returns them)
        cli.log("Haplotype read binning with k = %d: markers %s, %s; %d hap1 and %d hap2 markers, of %d and %d k-mers private to hap1 and to hap2" % (
            k, hap["markers"], "child threshold %d (%s)" % (thre, origin) if origin else "no child threshold", sm["selected"], sp["selected"],
            sm["candidates"] - sm["in_absent"], sp["candidates"] - sp["in_absent"]))
        select_line(HAP_BINS, (sm, sp))
    except BaseException:
        m.close()
        p.close()
        if child is not None:
            child.close()
        raise
    return m, p, sm["selected"], sp["selected"], child


def open_trio(hap, k, device, as_tables):
    """trio mode: the parents opened, their hap-mers counted, the first log line -> (mat, pat, thre_mat, thre_pat, M_total, P_total); the
    caller closes the tables.  as_tables (--marker-tables): the two hap-mer sets become tables of their own (marker_tables), the parents
    are closed, the totals are the selects', and what comes back is (M', P', 1, 1, ...): the same counts per read from far smaller tables"""
    from .table import KmerTable
    mat, pat, tm, tp = extensions.open_parents(hap, k, device)
    line = "Trio read binning with k = %%d: maternal threshold %%d (%s), paternal threshold %%d (%s); %%d maternal and %%d paternal hap-mers" % (
        "given" if hap["thre_mat"] is not None else "from the histogram", "given" if hap["thre_pat"] is not None else "from the histogram")
    if not as_tables:
        try:
            census = KmerTable.hapmer_census_parents(mat, pat, None, tm, tp)
            cli.log(line % (k, tm, tp, census.mat[0], census.pat[0]))
        except BaseException:
            mat.close()
            pat.close()
            raise
        return mat, pat, tm, tp, census.mat[0], census.pat[0]
    try:
        m, p, sm, sp = marker_tables(mat, pat, None, tm, tp, 1)
    finally:
        mat.close()
        pat.close()
    try:                                                # (from here on the marker tables are this function's until it returns them)
        cli.log(line % (k, tm, tp, sm["selected"], sp["selected"]))
        select_line(BINS, (sm, sp))
    except BaseException:
        m.close()
        p.close()
        raise
    return m, p, 1, 1, sm["selected"], sp["selected"]


def run(argv):
    a = parse_args(argv)
    reader = check_reader(a)
    gz, route = check_gz_route(a, reader)
    write_gz, deflate = check_write_gz(a)
    reads, k, device, hap, min_markers, batch_bases = check_flags(a)
    prefix = a["prefix"] if a["prefix"] is not None else reads[0]
    by_haps = "hap1" in hap
    names = HAP_BINS if by_haps else BINS
    check_write_jf(a, hap, prefix, names)
    reads_table = None
    if by_haps:
        mat, pat, m_total, p_total, reads_table = open_haps(hap, reads, k, device, keep_child=a["write_jf"])
        tm = tp = 1
    else:
        mat, pat, tm, tp, m_total, p_total = open_trio(hap, k, device, a["marker_tables"])
    try:
        (haps_totals_check if by_haps else check_totals)(m_total, p_total)
        t, timings = _Tables(mat, pat, tm, tp), {}
        jf = _WriteJf(t, reads_table, k, device, prefix, names, reads, reader, t.gz_open if gz == "device" else None) if a["write_jf"] else None
        try:
            per_bin, seconds = bin_files(reads, prefix, t.count, m_total, p_total, min_markers, a["paired"], a["per_read"], a["write_reads"], batch_bases, reader=reader,
                                         count_text=t.count_text, gz_open=t.gz_open if gz == "device" else None, route_text=t.route_text if route == "device" else None,
                                         timings=timings, write_gz=write_gz, deflate=t.deflate if write_gz and deflate == "device" else None, names=names, write_jf=jf)
        finally:
            timing_lines(timings, gz, route, deflate if write_gz else None)
    finally:
        mat.close()
        pat.close()
        if reads_table is not None:
            reads_table.close()
    n, bases = sum(r for r, _ in per_bin), sum(b for _, b in per_bin)
    cli.log("Read bins: " + "; ".join("%s %d reads (%s), %d bases (%s)" % (names[b], per_bin[b][0], _share(per_bin[b][0], n), per_bin[b][1], _share(per_bin[b][1], bases))
                                      for b in range(3)) + " in %s.readbins.tsv" % prefix)
    if jf is not None:
        jf.log(per_bin)
    extensions.device_line("[triobin] read_bins device seconds: %.6f; %s bases per second" % (seconds, "%.4g" % (bases / seconds) if seconds > 0 else "NA"))
    if reader == "device":
        extensions.device_line("[triobin] read_text index + pack device seconds: %.6f; %s text bytes per second" % (
            t.index_seconds, "%.4g" % (t.text_bytes / t.index_seconds) if t.index_seconds > 0 else "NA"))
    return 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[1:]))
