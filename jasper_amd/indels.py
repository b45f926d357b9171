"""Indel scan: the writers of `*.indels.tsv` and `*.indels*.vcf` (cli --indels, kmerqc --indels).

An extension: the reference repairs length errors inside its walk (src/jasper.py: fix_insert, fix_del, fix_same_base_del,
fix_same_base_insertion) and reports nothing.  The scan (KmerTable.indel_scan; semantics in include/jasper_hip.h,
jasper_indel_scan) lists the positions of the contigs where the reads hold a solid same-base insertion or a solid deletion of up
to `max_len` bytes: `het` when the contig's own sequence is solid there too (a length difference between the haplotypes), `error`
when only the alternative is (a length error the polisher has not repaired).

With the mixed half of the scan (`indel_scan(.., mixed=True)`, --indel-mixed; semantics: jasper_indel_scan_mixed) the insertions of
mixed bases are listed as well: three more columns in the TSV (mixed_het, mixed_error and complex, the sites where more than 64
prefixes of one length were solid and the search stopped) and more `TYPE=ins` lines in the VCF.

Limits: insertions of mixed bases are listed only with the mixed half, lengths above 16 are not listed, and two differences less than
k apart hide each other (the het-cluster half of the scan lists those where both alleles are solid: jasper_amd/hetclusters.py).

The scan reports every indel at its right-most position; the VCF writer moves it to the left-most one (`left_align`), as VCF asks.
Nothing here touches the GPU: the functions take names, lengths, sequences, counters and records.
"""
from .report import align, column_sums, contig_name, stage_table_text, vcf_preamble, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error\n"
KINDS = {1: "het", 2: "error"}
TYPES = {1: "ins", 2: "del"}
TYPE_NUMBERS = {"ins": 1, "del": 2}
MIXED_COLUMNS = "\tmixed_het\tmixed_error\tcomplex"
ZERO = (0, 0, 0, 0)
ZERO3 = (0, 0, 0)
_FOLD = {65: 65, 67: 67, 71: 71, 84: 84, 97: 65, 99: 67, 103: 71, 116: 84}      # ACGTacgt -> ACGT


def _row(name, stage, length, c):
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((name, stage, length) + tuple(c))


def totals(counts):
    """column sums of the (ins_het, ins_error, del_het, del_error) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 4)


def mixed_totals(mcounts):
    """column sums of the (mixed_het, mixed_error, complex) of the contigs that have any"""
    return column_sums(mcounts, 3)


def _more(c3):
    return "\t%d\t%d\t%d\n" % tuple(c3)


def indels_tsv_text(names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and four counters, or None for a contig
    that stage does not have (a row of zeros).  Per contig in the order of `names` one row per stage, then one row per stage for
    contig `*` with the sums.  Stages of the mixed scan are (stage name, lengths, counts, mixed counts): every row, the header
    included, then ends in the three columns mixed_het, mixed_error, complex."""
    if not any(len(st) > 3 for st in stages):
        return stage_table_text(TSV_HEADER, names, stages, _row, ZERO, totals)
    paired = []                                  # a contig's row: (counts, mixed counts -- zeros where a stage has none)
    for stage, lengths, counts, mc in (tuple(st) + (None,) * (4 - len(st)) for st in stages):
        paired.append((stage, lengths, [None if c is None else (c, mc[i] if mc is not None and mc[i] is not None else ZERO3) for i, c in enumerate(counts)]))
    return stage_table_text(TSV_HEADER[:-1] + MIXED_COLUMNS + "\n", names, paired, lambda name, stage, length, r: _row(name, stage, length, r[0])[:-1] + _more(r[1]),
                            (ZERO, ZERO3), lambda rows: (totals([r and r[0] for r in rows]), mixed_totals([r and r[1] for r in rows])))


def _letter(v):
    return v if isinstance(v, str) else chr(int(v))


def _rec_fields(r):
    """(seq, pos, type number, len, base, ref_min, alt_min, kind) of a record of IndelScan.records or of a tuple in the order of
    IndelScan.record_tuples()"""
    if hasattr(r, "dtype"):
        return (int(r["seq"]), int(r["pos"]), int(r["type"]), int(r["len"]), _letter(r["base"]), int(r["ref_min"]), int(r["alt_min"]), int(r["kind"]))
    seq, pos, typ, ln, base, rmin, amin, kind = r
    return int(seq), int(pos), TYPE_NUMBERS[typ] if isinstance(typ, str) else int(typ), int(ln), _letter(base), int(rmin), int(amin), int(kind)


def _bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else s


def left_align(seq, q, typ, length, base):
    """the left-most position of an indel the scan reported at q (0-based: the deleted bytes are seq[q .. q+length-1], the insertion
    lies before byte q).  A deletion moves to q - 1 while q > 1, seq[q-1] is a base and equals (case folded) seq[q+length-1]; an
    insertion of `base` repeated moves while q > 1 and seq[q-1] is that base.  typ: 1 / 'ins' or 2 / 'del'."""
    s = _bytes(seq)
    if typ in (1, "ins"):
        x = ord(_letter(base))
        while q > 1 and _FOLD.get(s[q - 1]) == x:
            q -= 1
    else:
        while q > 1 and _FOLD.get(s[q - 1]) is not None and _FOLD.get(s[q - 1]) == _FOLD.get(s[q + length - 1]):
            q -= 1
    return q


def _mixed_fields(r):
    """(seq, pos, len, y, ref_min, alt_min, kind) of a record of MixedInsertions.records or of a tuple in the order of its
    record_tuples()"""
    if hasattr(r, "dtype"):
        ln = int(r["len"])
        return (int(r["seq"]), int(r["pos"]), ln, "".join("ACGT"[(int(r["bases"]) >> (2 * i)) & 3] for i in range(ln)), int(r["ref_min"]), int(r["alt_min"]),
                int(r["kind"]))
    seq, pos, ln, y, rmin, amin, kind = r
    return int(seq), int(pos), int(ln), y if isinstance(y, str) else bytes(y).decode("latin-1"), int(rmin), int(amin), int(kind)


def left_align_mixed(seq, q, y):
    """the left-most form (q, y) of the insertion of the string y before byte q: while q > 1 and seq[q-1] is a base equal (case folded)
    to y's last base, y is rotated -- its last base moves to its front -- and q moves one to the left"""
    s = _bytes(seq)
    y = y.upper()
    while q > 1 and _FOLD.get(s[q - 1]) == ord(y[-1]):
        y = y[-1] + y[:-1]
        q -= 1
    return q, y


def vcf_lines(names, seqs, records, mixed_records=()):
    """[(seq, POS, type number, len, ALT, REF, INFO)] sorted: every record left-aligned, POS = the 1-based position of the anchor byte"""
    out = []
    for seq, pos, ln, y, rmin, amin, kind in (_mixed_fields(r) for r in mixed_records):
        s = _bytes(seqs[seq])
        q, y = left_align_mixed(s, pos, y)
        anchor = s[q - 1:q].decode("latin-1").upper()
        out.append((seq, q, 1, ln, anchor + y, anchor, "KIND=%s;TYPE=ins;LEN=%d;RC=%d;AC=%d" % (KINDS[kind], ln, rmin, amin)))
    for seq, pos, typ, ln, base, rmin, amin, kind in (_rec_fields(r) for r in records):
        s = _bytes(seqs[seq])
        q = left_align(s, pos, typ, ln, base)
        anchor = s[q - 1:q].decode("latin-1").upper()
        if typ == 1:
            ref, alt = anchor, anchor + base * ln
        else:
            ref, alt = anchor + s[q:q + ln].decode("latin-1").upper(), anchor
        out.append((seq, q, typ, ln, alt, ref, "KIND=%s;TYPE=%s;LEN=%d;RC=%d;AC=%d" % (KINDS[kind], TYPES[typ], ln, rmin, amin)))
    out.sort()
    return out


def vcf_text(k, thre, max_len, names, lengths, seqs, records, mixed_records=None):
    """VCFv4.2: one `##contig` line per contig in the order of `names`, then one line per record, left-aligned and ordered by (contig,
    POS, TYPE (ins before del), LEN, ALT) whatever order they come in: name, POS, ., REF, ALT, ., .,
    KIND=het|error;TYPE=ins|del;LEN=L;RC=ref_min;AC=alt_min.  seqs[i] = contig i's sequence (the anchor and the deleted bases are
    read from it).  mixed_records (not None: the scan had its mixed half) are the insertions of mixed bases: `TYPE=ins` lines in the
    same order, REF = the anchor, ALT = the anchor and the inserted string."""
    mixed = mixed_records is not None
    out = vcf_preamble("indel scan, k=%d, threshold=%d, max_len=%d%s" % (k, thre, max_len, ", mixed" if mixed else ""), names, lengths, [
        ("KIND", "String", "het: the contig's sequence and the alternative are both solid in the reads; error: only the alternative is"),
        ("TYPE", "String", "ins: the reads hold LEN more %s; del: the reads lack LEN bytes" % ("bases" if mixed else "copies of one base")),
        ("LEN", "Integer", "length of the insertion or deletion"),
        ("RC", "Integer", "smallest read count of the contig's k-mers that span the site"),
        ("AC", "Integer", "smallest read count of the k-mers of the alternative")])
    for seq, q, _typ, _ln, alt, ref, info in vcf_lines(names, seqs, records, mixed_records if mixed else ()):
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (names[seq], q, ref, alt, info))
    return "".join(out)


def stage_log_text(counts):
    """`A het and B error insertions, C het and D error deletions` of one stage"""
    return "%d het and %d error insertions, %d het and %d error deletions" % totals(counts)


def mixed_stage_log_text(mcounts):
    """`A het and B error mixed insertions, C complex sites` of one stage"""
    return "%d het and %d error mixed insertions, %d complex sites" % mixed_totals(mcounts)


def mixed_log_text(mcounts0, mcounts1):
    return "Mixed insertions: before polishing %s; after polishing %s" % (mixed_stage_log_text(mcounts0), mixed_stage_log_text(mcounts1))


def log_text(counts0, counts1):
    return "Indel scan: before polishing %s; after polishing %s" % (stage_log_text(counts0), stage_log_text(counts1))
