"""Compound scan: the writers of `*.compound.tsv` and `*.compound*.vcf` (cli --compound, kmerqc --compound).

An extension: the reference repairs clusters of differences inside its walk where it can and reports nothing.  Two differences less
than k apart hide each other from the variant and the indel scan: every window that covers one holds the contig's wrong base at the
other, so no single-edit alternative is solid.  What shows is a run of unreliable k-mers of k + R - 1 windows, R the bytes from the
first difference to the last.  The scan (KmerTable.compound_scan; semantics in include/jasper_hip.h, jasper_compound_scan) walks the
solid k-mers of the reads from the left flank of every such run with R <= max_len and lists each string of up to max_len bases that
rejoins the contig on the right flank: several substitutions (`TYPE=mnp`, as long as what it replaces) or a substitution and a length
error (`TYPE=complex`).  Every record is an error -- the contig's own k-mers there are unreliable.

Per contig the TSV counts the sites (runs that were searched), the bridged ones (at least one record), the records, the long runs
(R > max_len: not searched) and the complex sites (more than 64 prefixes of one length were solid: the search stopped there).

Limits: compound het sites are not listed here (where both alleles are solid there is no unreliable run) but by the het-cluster
half of the indel scan (--indels --het-clusters, jasper_amd/hetclusters.py), deletions alone stay the indel scan's and a single substitution the variant scan's, and nothing longer than 64 bases is listed.

Nothing here touches the GPU: the functions take names, lengths, sequences, counters and records.
"""
from .report import align, column_sums, contig_name, stage_table_text, vcf_preamble, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)
from .table import compound_string

TSV_HEADER = "#contig\tstage\tlength\tsites\tbridged\trecords\tlong\tcomplex\n"
ZERO = (0, 0, 0, 0, 0)
KIND_TEXT = "error: only the alternative is solid in the reads; the contig's own k-mers there are unreliable"


def _row(name, stage, length, c):
    return "%s\t%s" % (name, stage) + "\t%d" * (1 + len(c)) % ((length,) + tuple(c)) + "\n"


def totals(counts):
    """column sums of the (sites, bridged, records, long, complex) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 5)


def compound_tsv_text(names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and five counters, or None for a contig
    that stage does not have (a row of zeros).  Per contig in the order of `names` one row per stage, then one row per stage for
    contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, _row, ZERO, totals)


def _rec_fields(r):
    """(seq, pos, ref_len, len, y, ref_min, alt_min) of a record of CompoundScan.records or of a tuple in the order of
    CompoundScan.record_tuples()"""
    if hasattr(r, "dtype"):
        return (int(r["seq"]), int(r["pos"]), int(r["ref_len"]), int(r["len"]), compound_string(r["bases"], r["len"]), int(r["ref_min"]), int(r["alt_min"]))
    seq, pos, rlen, ln, y, rmin, amin = r
    return int(seq), int(pos), int(rlen), int(ln), y if isinstance(y, str) else bytes(y).decode("latin-1"), int(rmin), int(amin)


def _by_len_alt(seq, pos1, rlen, ln, alt):
    return seq, pos1, ln, alt


def vcf_lines(seqs, records, kind="error", order=_by_len_alt):
    """[(seq, POS, ALT, REF, INFO)] of the replacements, here and in jasper_amd/hetclusters.py, sorted by order(seq, POS, RLEN, LEN, ALT) --
    here (contig, POS, LEN, ALT): POS = a + 1, REF = the contig's R bytes as they stand"""
    out = []
    for seq, pos, rlen, ln, y, rmin, amin in (_rec_fields(r) for r in records):
        s = seqs[seq]
        ref = s[pos:pos + rlen]
        ref = ref if isinstance(ref, str) else bytes(ref).decode("latin-1")
        out.append((order(seq, pos + 1, rlen, ln, y), ref, "KIND=%s;TYPE=%s;RLEN=%d;LEN=%d;RC=%d;AC=%d" % (kind, "mnp" if rlen == ln else "complex", rlen, ln, rmin, amin)))
    out.sort()
    return [(key[0], key[1], key[-1], ref, info) for key, ref, info in out]


def vcf_text(k, thre, max_len, names, lengths, seqs, records, scan="compound scan", kind="error", kind_text=KIND_TEXT, order=_by_len_alt):
    """VCFv4.2: one `##contig` line per contig in the order of `names`, then one line per record ordered by (contig, POS, LEN, ALT)
    whatever order they come in: name, POS, ., REF, ALT, ., ., KIND=error;TYPE=mnp|complex;RLEN=R;LEN=t;RC=ref_min;AC=alt_min.
    seqs[i] = contig i's sequence: REF is read from it.  Both alleles are non-empty, so there is no anchor base.
    scan, kind, kind_text and order: what jasper_amd/hetclusters.py writes its own file with."""
    out = vcf_preamble("%s, k=%d, threshold=%d, max_len=%d" % (scan, k, thre, max_len), names, lengths, [
        ("KIND", "String", kind_text),
        ("TYPE", "String", "mnp: ALT is as long as REF; complex: the lengths differ"),
        ("RLEN", "Integer", "bytes of the contig that are replaced"),
        ("LEN", "Integer", "bases the reads hold in their place"),
        ("RC", "Integer", "smallest read count of the contig's k-mers that span the site"),
        ("AC", "Integer", "smallest read count of the k-mers of the alternative")])
    for seq, pos1, alt, ref, info in vcf_lines(seqs, records, kind, order):
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (names[seq], pos1, ref, alt, info))
    return "".join(out)


def stage_log_text(counts):
    """`A sites, B bridged, C records, D long runs, E complex sites` of one stage"""
    return "%d sites, %d bridged, %d records, %d long runs, %d complex sites" % totals(counts)


def log_text(counts0, counts1):
    return "Compound scan: before polishing %s; after polishing %s" % (stage_log_text(counts0), stage_log_text(counts1))
