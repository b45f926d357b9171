"""Het clusters: the writers of `*.het_clusters.tsv` and `*.het_clusters*.vcf` (cli --indels --het-clusters, kmerqc likewise).

An extension: the reference reports nothing of the kind.  Two heterozygous differences less than k apart hide each other from the
variant and the indel scan: the candidate at the left one is there, but every later window that covers it also covers the right one,
where the contig holds the other haplotype's allele, so every single-edit check rejects it.  The het-cluster half of the indel scan
(KmerTable.indel_scan(.., clusters=N); semantics in include/jasper_hip.h, jasper_indel_scan_clusters) walks the solid k-mers of the
reads from every such candidate whose own contig k-mers are solid too, and lists each string of up to N bases that rejoins the contig
within N bytes: several substitutions (`TYPE=mnp`, as long as what it replaces) or a substitution beside a length difference
(`TYPE=complex`).  Every record is het -- the contig's own k-mers there are solid by construction.

Per contig the TSV counts the candidates that were searched, the sites (searched candidates with at least one record), the records
and the complex candidates (more than 64 prefixes of one length were solid: the search stopped there).

Limits: a cluster where the contig's own k-mers are unreliable is the compound scan's (`--compound`), a single substitution stays the
variant scan's and a pure insertion or deletion the indel scan's, and nothing longer than 64 bases is listed.

Nothing here touches the GPU: the functions take names, lengths, sequences, counters and records.
"""
from . import compound
from .report import align, column_sums, contig_name, stage_table_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\tsearched\tsites\trecords\tcomplex\n"
ZERO = (0, 0, 0, 0)


def totals(counts):
    """column sums of the (searched, sites, records, complex) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 4)


def het_clusters_tsv_text(names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and four counters, or None for a contig
    that stage does not have (a row of zeros).  Per contig in the order of `names` one row per stage, then one row per stage for
    contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, compound._row, ZERO, totals)


def _by_rlen_len_alt(seq, pos1, rlen, ln, alt):
    return seq, pos1, rlen, ln, alt


def vcf_lines(seqs, records):
    """[(seq, POS, ALT, REF, INFO)] sorted by (contig, POS, RLEN, LEN, ALT): POS = p + 1, REF = the contig's R bytes as they stand"""
    return compound.vcf_lines(seqs, records, "het", _by_rlen_len_alt)


def vcf_text(k, thre, max_len, names, lengths, seqs, records):
    """VCFv4.2: one `##contig` line per contig in the order of `names`, then one line per record ordered by (contig, POS, RLEN, LEN,
    ALT) whatever order they come in: name, POS, ., REF, ALT, ., ., KIND=het;TYPE=mnp|complex;RLEN=R;LEN=t;RC=ref_min;AC=alt_min.
    seqs[i] = contig i's sequence: REF is read from it.  Both alleles are non-empty, so there is no anchor base."""
    return compound.vcf_text(k, thre, max_len, names, lengths, seqs, records, "het-cluster scan", "het",
                             "het: the contig's sequence and the alternative are both solid in the reads", _by_rlen_len_alt)


def stage_log_text(counts):
    """`A searched, B sites, C records, D complex` of one stage"""
    return "%d searched, %d sites, %d records, %d complex" % totals(counts)


def log_text(counts0, counts1):
    return "Het clusters: before polishing %s; after polishing %s" % (stage_log_text(counts0), stage_log_text(counts1))
