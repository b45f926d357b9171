"""Both haplotypes of a diploid assembly evaluated together: the numbers derived from `KmerTable.spectrum_pair` and
`KmerTable.pair_scan` and the writers of `*.spectra_asm.tsv`, `*.diploid.completeness.tsv`, `*.diploid.tsv` and
`*.private.{asm,alt}.bed` (kmerqc --alt).

An extension: the reference has no counterpart.  Each haplotype on its own against all the reads stops near the homozygous share of
completeness and calls every k-mer of the other haplotype missing; the two FASTA files concatenated give the joint numbers and lose
the per-haplotype ones.  Here the reads' table R is joined with the tables of both haplotypes at once, and each haplotype's contigs
are scanned against R and the OTHER haplotype's table.

The pair spectrum is a matrix P of 4 rows (include/jasper_hip.h, jasper_table_spectrum_pair): row j = (k-mer in asm ? 1 : 0) |
(k-mer in alt ? 2 : 0), column c = min(count in the reads, 10001); P[j][c] for c >= 1 counts distinct k-mers of the reads, P[j][0]
for j >= 1 the distinct k-mers of the two haplotypes that the reads do not hold.  A set of haplotypes is a set of rows: asm = rows 1
and 3, alt = rows 2 and 3, both = rows 1, 2 and 3.

A window of a haplotype's contig is private when the other haplotype does not hold its k-mer: private_solid when the reads hold it
`threshold` times or more (the haplotypes differ there, and the reads support this one's allele), private_weak when they do not (an
error only this haplotype has).  An unreliable window that is not private is an unsupported k-mer both haplotypes hold.

Nothing here touches the GPU: the functions take a PairSpectrum, a numpy array or a list of rows, and names, lengths, counters and runs.
"""
from .report import column_sums, qv_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic: `.tmp`, then renamed)

ROWS = 4
COLS = 10002
CLASS_LABELS = ("reads_only", "asm_only", "alt_only", "shared")
SETS = (("asm", (1, 3)), ("alt", (2, 3)), ("both", (1, 2, 3)))
KIND_LABELS = {1: "solid", 2: "weak"}
SPECTRA_HEADER = "#class\tread_count\tkmers\n"
COMPLETENESS_HEADER = "#set\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tdistinct\tnot_in_reads\n"
TSV_HEADER = ("#set\tcontig\tlength\twindows\tvalid\tunreliable\tabsent\tQV_unreliable\tQV_absent\tprivate_solid\tprivate_weak\tshared_unreliable"
              "\tprivate_fraction\n")


def cells_of(pair):
    """the matrix as a list of ROWS lists of Python ints (pair: PairSpectrum, numpy array or list of rows)"""
    cells = getattr(pair, "cells", pair)
    rows = [[int(v) for v in row] for row in cells]
    if len(rows) != ROWS or any(len(r) != len(rows[0]) for r in rows) or not rows[0]:
        raise ValueError("a pair spectrum has %d rows of equal length" % ROWS)
    return rows


def spectra_asm_text(pair):
    """header, then one row per non-zero cell ordered by (class, column): class (reads_only, asm_only, alt_only, shared), read_count
    (the column: 0 = not in the reads, the last column = that count or more), kmers"""
    out = [SPECTRA_HEADER]
    for j, row in enumerate(cells_of(pair)):
        for c, v in enumerate(row):
            if v:
                out.append("%s\t%d\t%d\n" % (CLASS_LABELS[j], c, v))
    return "".join(out)


def completeness_pct(found, solid):
    """100 * found / solid, "%.4f"; "NA" when there is no solid k-mer"""
    if solid <= 0:
        return "NA"
    return "%.4f" % (100.0 * float(found) / float(solid))


def completeness_rows(pair, threshold):
    """[(set, threshold, solid, found, distinct, not_in_reads)] for asm, alt and both, with t = max(1, threshold) (a k-mer the reads do
    not hold is never solid): solid = distinct k-mers of the reads with count >= t, found = those of them the set holds, distinct =
    distinct k-mers of the set, not_in_reads = those the reads do not hold"""
    rows = cells_of(pair)
    t = max(1, int(threshold))
    solid = sum(sum(r[t:]) for r in rows)
    return [(name, t, solid, sum(sum(rows[j][t:]) for j in js), sum(sum(rows[j]) for j in js), sum(rows[j][0] for j in js)) for name, js in SETS]


def completeness_text(k, rows):
    """rows: completeness_rows' -> header and one line per row"""
    out = [COMPLETENESS_HEADER]
    for name, thr, solid, found, distinct, not_in_reads in rows:
        out.append("%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (name, k, thr, solid, found, completeness_pct(found, solid), distinct, not_in_reads))
    return "".join(out)


def private_fraction(c):
    """(private_solid + private_weak) / valid, "%.4f"; "NA" without a valid window"""
    _, v, _, _, ps, pw = c
    if v <= 0:
        return "NA"
    return "%.4f" % (float(ps + pw) / float(v))


def _row(which, name, length, c, k):
    w, v, u, a, ps, pw = c
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%s\n" % (which, name, length, w, v, u, a, qv_text(u, v, k), qv_text(a, v, k), ps, pw, u - pw, private_fraction(c))


def totals(counts):
    """column sums of the contigs' (windows, valid, unreliable, absent, private_solid, private_weak)"""
    return column_sums([tuple(c) for c in counts], 6)


def diploid_tsv_text(k, haplotypes):
    """haplotypes: [(set name, contig names, lengths, counts)] for asm and alt, counts[i] = contig i's (windows, valid, unreliable,
    absent, private_solid, private_weak).  Per haplotype its contigs in input order and then contig `*` with the sums; at the end
    `both *`, the sum of the `*` rows.  QV is report.qv_text's; shared_unreliable = unreliable - private_weak."""
    out = [TSV_HEADER]
    star = []
    for which, names, lengths, counts in haplotypes:
        for name, length, c in zip(names, lengths, counts):
            out.append(_row(which, name, length, c, k))
        star.append((sum(lengths), totals(counts)))
        out.append(_row(which, "*", star[-1][0], star[-1][1], k))
    out.append(_row("both", "*", sum(ln for ln, _ in star), totals([c for _, c in star]), k))
    return "".join(out)


def run_fields(r):
    """(seq, start, n_kmers, kind, sum_reads) of a run: a record of PairScan.runs or such a tuple"""
    if hasattr(r, "dtype"):
        return tuple(int(r[f]) for f in ("seq", "start", "n_kmers", "kind", "sum_reads"))
    return tuple(int(v) for v in r)


def bed_text(k, names, runs):
    """one line per run, seq indexing `names`: contig start end kind n_kmers mean_reads, end = start + n_kmers + k - 1, kind = solid or
    weak, mean_reads = sum_reads / n_kmers ("%.2f").  Every run is listed."""
    out = []
    for r in runs:
        seq, start, nk, kind, sr = run_fields(r)
        out.append("%s\t%d\t%d\t%s\t%d\t%.2f\n" % (names[seq], start, start + nk + k - 1, KIND_LABELS[kind], nk, float(sr) / float(nk)))
    return "".join(out)


def completeness_log_text(rows):
    """the log line of the three completeness rows (without its prefix)"""
    def pct(found, solid):
        p = completeness_pct(found, solid)
        return p if p == "NA" else p + " %"
    thr, solid = rows[0][1], rows[0][2]
    return "k-mer completeness: %s (%d of %d solid k-mers, threshold %d)" % (
        ", ".join("%s %s" % (name, pct(found, solid)) for name, _, _, found, _, _ in rows), rows[-1][3], solid, thr)


def qv_log_text(k, asm_counts, alt_counts):
    """the log line of the dense QV (unreliable k-mers) of asm, alt and both"""
    a, b = totals(asm_counts), totals(alt_counts)
    both = totals([a, b])
    return "dense k-mer QV (unreliable k-mers): %s" % ", ".join("%s %s" % (name, qv_text(c[2], c[1], k)) for name, c in (("asm", a), ("alt", b), ("both", both)))


def private_log_text(asm_counts, asm_runs, alt_counts, alt_runs):
    """the log line of the private windows and the listed runs of each haplotype"""
    a, b = totals(asm_counts), totals(alt_counts)
    return "private windows: asm %d solid %d weak in %d runs; alt %d solid %d weak in %d runs" % (a[4], a[5], len(asm_runs), b[4], b[5], len(alt_runs))
