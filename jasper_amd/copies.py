"""Copy-number scan: the single-copy peak of the reads' histogram and the writers of `*.copies.tsv` and `*.copies*.bed`
(cli --copies, kmerqc --copies).

An extension: the reference has no counterpart.  The spectrum (jasper_amd/spectra.py) counts the distinct k-mers that the
assembly holds more or fewer times than the reads support; the scan (KmerTable.copy_report; semantics in include/jasper_hip.h,
jasper_copy_report) says WHERE they are: per contig how many windows are `excess` (the reads support more copies than the
assembly holds: a collapsed repeat) or `deficit` (the assembly holds more copies than the reads support: a duplicated
haplotig, or thin support), and the maximal runs of either class as a BED track.

Nothing here touches the GPU: the functions take names, lengths, counters and runs.
"""
from .report import align, column_sums, contig_name, stage_table_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\texcess\tdeficit\tsum_reads\tsum_asm\tdepth\tpeak\n"
KINDS = {1: "excess", 2: "deficit"}
ZERO = (0, 0, 0, 0, 0, 0)


def histogram_from_rows(rows):
    """the 10002 bins of jasper_histogram from rows (multiplicity, ..., n_distinct) as `jellyfish histo` prints them"""
    h = [0] * 10002
    for row in rows:
        m = int(row[0])
        h[min(max(m, 0), 10001)] += int(row[-1])
    return h


def peak_from_histogram(h10002, thre):
    """the read count of a k-mer present once in the genome: the smallest c in [max(thre, 2), 10000] with the largest h[c]; None
    when all those bins are 0 (bin 10001 is "that count or more" and bin 1 the errors: neither can be the peak)"""
    best, best_n = None, 0
    for c in range(max(int(thre), 2), min(len(h10002), 10001)):
        n = int(h10002[c])
        if n > best_n:
            best, best_n = c, n
    return best


def depth_text(sum_reads, sum_asm, peak):
    """sum_reads / (peak * sum_asm), "%.4f": 1 = the reads support what the assembly holds, above 1 collapsed, near 0.5 a
    duplicated haplotig; "NA" when the assembly's table has none of the windows' k-mers"""
    if sum_asm <= 0:
        return "NA"
    return "%.4f" % (float(sum_reads) / (float(peak) * float(sum_asm)))


def _row(name, stage, length, c, peak):
    w, v, e, d, sr, sa = c
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (name, stage, length, w, v, e, d, sr, sa, depth_text(sr, sa, peak), peak)


def totals(counts):
    """column sums of the (windows, valid, excess, deficit, sum_reads, sum_asm) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 6)


def copies_tsv_text(peak, names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and six counters, or None for a contig
    that stage does not have (a row of zeros and NA).  Per contig in the order of `names` one row per stage, then one row per
    stage for contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, lambda name, stage, length, c: _row(name, stage, length, c, peak), ZERO, totals)


def _run_fields(r):
    if hasattr(r, "dtype"):
        return tuple(int(r[f]) for f in ("seq", "start", "n_kmers", "kind", "sum_reads", "sum_asm"))
    return tuple(int(v) for v in r)


def listed(runs, min_run):
    """the runs (seq, start, n_kmers, kind, sum_reads, sum_asm) of at least min_run windows"""
    return [f for f in (_run_fields(r) for r in runs) if f[2] >= min_run]


def bed_text(k, peak, names, runs, min_run=1):
    """one line per run of at least min_run windows, seq indexing `names`:
    contig start end kind n_kmers mean_reads mean_asm read_copies, end = start + n_kmers + k - 1, kind = excess / deficit, the means
    = sum_reads / n_kmers and sum_asm / n_kmers, read_copies = sum_reads / (peak * n_kmers): the copies the reads support"""
    out = []
    for seq, start, nk, kind, sr, sa in listed(runs, min_run):
        out.append("%s\t%d\t%d\t%s\t%d\t%.2f\t%.2f\t%.2f\n" % (names[seq], start, start + nk + k - 1, KINDS[kind], nk, float(sr) / nk, float(sa) / nk,
                                                            float(sr) / (float(peak) * nk)))
    return "".join(out)


def peak_log_text(peak, given):
    return "Copy-number scan: single-copy read count (peak) is %d (%s)" % (peak, "given by --peak" if given else "from the k-mer histogram")


def stage_log_text(counts, n_listed):
    """`N excess and M deficit windows, R runs listed` of one stage"""
    t = totals(counts)
    return "%d excess and %d deficit windows, %d runs listed" % (t[2], t[3], n_listed)
