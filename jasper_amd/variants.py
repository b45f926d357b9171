"""Variant scan: the writers of `*.variants.tsv` and `*.variants*.vcf` (cli --variants, kmerqc --variants).

An extension: the reference meets heterozygous sites and leftover substitutions inside its walk (src/jasper.py: fixdiploid,
fix_k_case_sub), acts on them there and reports nothing.  The scan (KmerTable.variant_scan; semantics in include/jasper_hip.h,
jasper_variant_scan) lists the positions of the contigs where the reads hold a solid single-base alternative: `het` when the
contig's own base is solid too (the second allele of a diploid genome, which a one-haplotype assembly cannot show), `error` when
only the alternative is (a substitution the polisher has not made).

Limits: only isolated substitutions are listed.  Two differences less than k apart hide each other, because every k-mer that
covers one of them holds the other allele of the other; insertions and deletions are listed by the indel scan (jasper_amd/indels.py,
--indels; insertions of mixed bases with --indel-mixed), which leaves out lengths above 16 and, again, differences less than k apart.

Nothing here touches the GPU: the functions take names, lengths, counters and records.
"""
from .report import align, column_sums, contig_name, stage_table_text, vcf_preamble, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\tevaluated\thet\terror\thet_per_kb\n"
KINDS = {1: "het", 2: "error"}
ZERO = (0, 0, 0)


def het_per_kb_text(het, evaluated):
    """1000 het / evaluated, "%.4f"; "NA" when no position was evaluated"""
    if evaluated <= 0:
        return "NA"
    return "%.4f" % (1000.0 * float(het) / float(evaluated))


def _row(name, stage, length, c):
    ev, het, err = c
    return "%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (name, stage, length, ev, het, err, het_per_kb_text(het, ev))


def totals(counts):
    """column sums of the (evaluated, het, error) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 3)


def variants_tsv_text(names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and three counters, or None for a contig
    that stage does not have (a row of zeros and NA).  Per contig in the order of `names` one row per stage, then one row per
    stage for contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, _row, ZERO, totals)


def _letter(v):
    return v if isinstance(v, str) else chr(int(v))


def _rec_fields(r):
    """(seq, pos, ref, alt, ref_min, alt_min, kind) of a record of VariantScan.records or of a tuple in that order"""
    if hasattr(r, "dtype"):
        return int(r["seq"]), int(r["pos"]), _letter(r["ref"]), _letter(r["alt"]), int(r["ref_min"]), int(r["alt_min"]), int(r["kind"])
    seq, pos, ref, alt, rmin, amin, kind = r
    return int(seq), int(pos), _letter(ref), _letter(alt), int(rmin), int(amin), int(kind)


def vcf_text(k, thre, names, lengths, records):
    """VCFv4.2: one `##contig` line per contig in the order of `names`, then one line per record, sorted by (seq, pos, alt) whatever
    order they come in: name, pos + 1 (VCF positions are 1-based), ., REF, ALT, ., ., KIND=het|error;RC=ref_min;AC=alt_min"""
    out = vcf_preamble("variant scan, k=%d, threshold=%d" % (k, thre), names, lengths, [
        ("KIND", "String", "het: the contig's base and the alternative are both solid in the reads; error: only the alternative is"),
        ("RC", "Integer", "smallest read count of the k k-mers that cover the position, with the contig's base"),
        ("AC", "Integer", "smallest read count of those k-mers with the alternative base")])
    for seq, pos, ref, alt, rmin, amin, kind in sorted(_rec_fields(r) for r in records):
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\tKIND=%s;RC=%d;AC=%d\n" % (names[seq], pos + 1, ref, alt, KINDS[kind], rmin, amin))
    return "".join(out)


def stage_log_text(counts):
    """`N het and M error sites` of one stage"""
    t = totals(counts)
    return "%d het and %d error sites" % (t[1], t[2])


def log_text(counts0, counts1):
    return "Variant scan: before polishing %s; after polishing %s" % (stage_log_text(counts0), stage_log_text(counts1))
