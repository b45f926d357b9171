"""The read-text path's parser restated line by line in plain Python (include/jasper_hip.h: jasper_read_text_bins), and the crafted texts
its tests run on.  Nothing here is taken from jasper_amd.

parse(text, eof, fmt) -> (used, rec_start, head_end, lens, seq) or raises Bad(record, what):

    line    ends at a line feed; with eof a last line without one counts.  A CR directly before the line's end is not part of the line
    fastq   four lines a record, counted from the first byte: '@...', sequence, '+...', quality as long as the sequence.  Without eof a
            trailing partial record is left; with eof a line count that is no multiple of 4 is the first verdict, on record lines // 4
    fasta   a line that begins with '>' is a header; a record is a header and the lines up to the next header, its sequence their bytes
            without line ends.  Without eof the last record is left
    used    the bytes whole records cover; rec_start has one entry per record and `used` behind them; head_end[i] = where record i's
            header line ends (before a CR); seq = the sequences back to back"""
import readbins_ref as ref

ENDS_INSIDE = "the file ends inside it"
NO_AT = "its first line does not begin with @"
NO_PLUS = "its third line does not begin with +"
UNEQUAL = "its quality line is not as long as its sequence"
BLOCK = 4096                    # text bytes of a workgroup of the kernels (readtext_plan.hpp: RT_BLOCK)
SCAN_PASS_BLOCKS = 1024         # block totals one pass of the block-total scan takes (readtext_plan.hpp: RT_SCAN_PASS)
K = ref.TRIO_K


class Bad(Exception):
    def __init__(self, record, what):
        Exception.__init__(self, "record %d: %s" % (record, what))
        self.record, self.what = record, what


def lines_of(text, eof):
    """[(start, end without CR, start of the next line)]"""
    out, pos, n = [], 0, len(text)
    while pos < n:
        lf = text.find(b"\n", pos)
        if lf < 0 and not eof:
            break
        end, nxt = (n, n) if lf < 0 else (lf, lf + 1)
        out.append((pos, end - 1 if end > pos and text[end - 1] == 13 else end, nxt))
        pos = nxt
    return out


def parse(text, eof, fmt):
    text = bytes(text)
    ls = lines_of(text, eof)
    rec_start, head_end, lens, seq = [], [], [], []
    if fmt == "fastq":
        n = len(ls) // 4
        if eof and len(ls) % 4:
            raise Bad(n, ENDS_INSIDE)
        for i in range(n):
            (hs, he, _), (ss, se, _), (ps, _, _), (qs, qe, _) = ls[4 * i:4 * i + 4]
            if text[hs:hs + 1] != b"@":
                raise Bad(i, NO_AT)
            if text[ps:ps + 1] != b"+":
                raise Bad(i, NO_PLUS)
            if qe - qs != se - ss:
                raise Bad(i, UNEQUAL)
            rec_start.append(hs)
            head_end.append(he)
            lens.append(se - ss)
            seq.append(text[ss:se])
        used = ls[4 * n - 1][2] if n else 0
    else:
        heads = [j for j, (s, _, _) in enumerate(ls) if text[s:s + 1] == b">"]
        assert not ls or heads[:1] == [0], "the text must begin with a header"
        n = max(0, len(heads) - (0 if eof else 1))
        for i in range(n):
            upto = heads[i + 1] if i + 1 < len(heads) else len(ls)
            body = b"".join(text[s:e] for s, e, _ in ls[heads[i] + 1:upto])
            rec_start.append(ls[heads[i]][0])
            head_end.append(ls[heads[i]][1])
            lens.append(len(body))
            seq.append(body)
        used = 0 if n == 0 else ls[heads[n]][0] if n < len(heads) else len(text)
    return used, rec_start + [used], head_end, lens, b"".join(seq)


def reads_of(lens, seq):
    out, at = [], 0
    for ln in lens:
        out.append(seq[at:at + ln])
        at += ln
    return out


# ---- the crafted texts ------------------------------------------------------------------------------------------------------------
def record(name, s, eol=b"\n", qual=None):
    return b"@" + name + eol + s + eol + b"+" + eol + (b"I" * len(s) if qual is None else qual) + eol


def base_records(trio, eol=b"\n"):
    """(a) with (c): 80 reads of the trio's R1 as FASTQ records, and among them an empty read with an empty quality line, reads of k - 1
    and of k bases, quality lines that begin with @ and with +, a lone CR inside a sequence, lower case and N"""
    r1 = [s for _, s in trio["r1"] if len(s) == 150][:80]
    recs = [record(b"r%d len=%d" % (i, len(s)), s, eol) for i, s in enumerate(r1)]
    recs[7] = record(b"empty", b"", eol)
    recs[19] = record(b"short", r1[19][:K - 1], eol)
    recs[20] = record(b"one_window", r1[20][:K], eol)
    recs[33] = record(b"qual_at", r1[33], eol, b"@" + b"I" * 149)
    recs[34] = record(b"qual_plus", r1[34], eol, b"+" + b"I" * 149)
    recs[46] = record(b"lone_cr", r1[46][:70] + b"\r" + r1[46][70:], eol)
    recs[58] = record(b"lower", r1[58][:40] + r1[58][40:110].lower() + r1[58][110:], eol)
    recs[59] = record(b"with_n", r1[59][:75] + b"N" + r1[59][76:], eol)
    return recs


def fasta_text(trio, eol=b"\n"):
    """(f): one-line records, records of several lines of unequal lengths, blank lines, a header alone, `>` inside a sequence line"""
    r2 = [s for _, s in trio["r2"] if len(s) == 150][:40]
    out = []
    for i, s in enumerate(r2):
        if i % 4 == 0:
            out.append(b">one%d" % i + eol + s + eol)
        elif i % 4 == 1:
            out.append(b">three%d x" % i + eol + s[:60] + eol + s[60:110] + eol + s[110:] + eol)
        elif i % 4 == 2:
            out.append(b">blank%d" % i + eol + s[:80] + eol + eol + s[80:] + eol + eol)
        else:
            out.append(b">gt%d" % i + eol + s[:30] + b">" + s[31:] + eol)
        if i == 10:
            out.append(b">header_only" + eol)
    return b"".join(out)


def cases(trio):
    """[(name, fmt, text, eof)]: every text the CPU and the GPU test parse; the malformed ones are in malformed()"""
    recs = base_records(trio)
    a = b"".join(recs)
    crlf = b"".join(base_records(trio, b"\r\n"))
    out = [("a", "fastq", a, True), ("a_not_eof", "fastq", a, False), ("b_crlf", "fastq", crlf, True), ("b_no_last_lf", "fastq", a[:-1], True),
           ("b_last_cr_no_lf", "fastq", crlf[:-1], True)]
    last = len(a) - len(recs[-1])
    for ln, at in enumerate(last_record_cuts(recs[-1])):                       # (d)
        out.append(("d_cut_in_line%d" % ln, "fastq", a[:last + at], False))
    out.append(("d_cut_after_record", "fastq", a[:last], False))
    hap = trio["hap_a"]
    long_read = hap[100:100 + 3 * BLOCK + 5]
    out.append(("e_long_read", "fastq", record(b"before", hap[:150]) + record(b"long", long_read) + record(b"after", hap[300:450]), True))
    fa = fasta_text(trio)
    out += [("f_fasta", "fasta", fa, True), ("f_fasta_not_eof", "fasta", fa, False), ("f_fasta_crlf", "fasta", fasta_text(trio, b"\r\n"), True),
            ("f_fasta_no_last_lf", "fasta", fa[:-1], True), ("f_fasta_cut", "fasta", fa[:len(fa) // 2], False)]
    reps = SCAN_PASS_BLOCKS * BLOCK // len(a) + 2
    out.append(("h_long_text", "fastq", a * reps, True))
    return out


def last_record_cuts(rec):
    """a cut position inside each of the four lines of a record (relative to its first byte)"""
    ends = [i for i, c in enumerate(rec) if c == 10]
    starts = [0] + [e + 1 for e in ends[:-1]]
    return [s + max(1, (e - s) // 2) if e > s else s for s, e in zip(starts, ends)]


def malformed(trio):
    """(g): [(name, text, eof, the verdict)], one per verdict of the host parser and one with two bad records; each bad record lies
    beyond the first block of the text"""
    recs = base_records(trio)
    at = 40

    def with_record(i, rec, rs=None):
        rs = list(recs if rs is None else rs)
        rs[i] = rec
        return rs

    no_at = with_record(at, b"X" + recs[at][1:])
    lines = recs[at].split(b"\n")
    no_plus = with_record(at, b"\n".join([lines[0], lines[1], b"-", lines[3], b""]))
    unequal = with_record(at, recs[at][:-2] + b"\n")
    two = with_record(60, b"X" + recs[60][1:], unequal)
    a = b"".join(recs)
    return [("g_no_at", b"".join(no_at), True, NO_AT), ("g_no_plus", b"".join(no_plus), True, NO_PLUS), ("g_unequal", b"".join(unequal), False, UNEQUAL),
            ("g_ends_inside", a[:a.rindex(b"\n", 0, len(a) - 1) + 1], True, ENDS_INSIDE), ("g_first_of_two", b"".join(two), True, UNEQUAL)]
