"""Duplication map: the writers of `*.dups.tsv`, `*.dups*.bed` and `*.dups.pairs.tsv` (cli --dups, kmerqc --dups).

An extension: the reference has no counterpart.  The copy scan (jasper_amd/copies.py) says where the assembly holds a stretch more
often than the reads support; the map (KmerTable.dup_map; semantics in include/jasper_hip.h, jasper_dup_map) says WHICH other place
holds the second copy: every window whose k-mer the assembly holds exactly twice is paired with the place of the other copy, and
the maximal colinear runs of such pairs are listed with what the reads say about them -- `read_copies` near 1 where the reads
support one copy of the two, near 2 where they support both.  No verdict is given: the files hold what the reads and the assembly
say.

Nothing here touches the GPU: the functions take names, lengths, counters and runs.
"""
from .report import align, column_sums, contig_name, stage_table_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\ttwo_copy\tdeficit\tmulti\tunplaced\tread_copies\tbest_mate\tbest_windows\tbest_fraction\n"
PAIRS_HEADER = "#stage\tcontig\tmate\tstrand\truns\twindows\tdeficit\tread_copies\n"
STRANDS = {0: "+", 1: "-"}
ZERO = (0, 0, 0, 0, 0, 0, 0, ".", 0)


def _run_fields(r):
    if hasattr(r, "dtype"):
        return tuple(int(r[f]) for f in ("seq", "start", "n_kmers", "mate_seq", "mate_start", "strand", "sum_reads", "n_deficit"))
    return tuple(int(v) for v in r)


def listed(runs, min_run):
    """the runs (seq, start, n_kmers, mate_seq, mate_start, strand, sum_reads, n_deficit) of at least min_run windows"""
    return [f for f in (_run_fields(r) for r in runs) if f[2] >= min_run]


def copies_text(sum_reads, peak, windows):
    """sum_reads / (peak * windows), "%.2f": the copies the reads support, of the two the assembly holds; "NA" without a window"""
    if windows <= 0:
        return "NA"
    return "%.2f" % (float(sum_reads) / (float(peak) * float(windows)))


def best_mates(names, runs):
    """per contig (name of the sequence that holds most of its mates, how many windows): runs of every length count, a tie goes to
    the first sequence in input order, (".", 0) for a contig without a run"""
    per = [{} for _ in names]
    for seq, _, nk, mate, _, _, _, _ in listed(runs, 1):
        per[seq][mate] = per[seq].get(mate, 0) + nk
    out = []
    for d in per:
        if not d:
            out.append((".", 0))
            continue
        best = min(d, key=lambda m: (-d[m], m))
        out.append((names[best], d[best]))
    return out


def extended(counts, names, runs):
    """a stage's rows: per contig its seven counters followed by (best_mate, best_windows)"""
    return [tuple(c) + b for c, b in zip(counts, best_mates(names, runs))]


def totals(rows):
    """column sums of the seven counters and of best_windows over the contigs that have any (None = contig missing)"""
    return column_sums(rows, 7) + (".", sum(r[8] for r in rows if r is not None))


def _row(name, stage, length, r, peak):
    w, v, two, de, mu, un, sr, best, bw = r
    frac = "%.4f" % (float(bw) / v) if v > 0 else "NA"
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%s\n" % (name, stage, length, w, v, two, de, mu, un, copies_text(sr, peak, two), best, bw, frac)


def dups_tsv_text(peak, names, stages):
    """stages: [(stage name, lengths, rows)], rows[i] = extended() of contig i, or None for a contig that stage does not have (a row
    of zeros, NA and `.`).  Per contig in the order of `names` one row per stage, then one row per stage for contig `*` with the
    sums (best_mate `.`, best_windows the sum of the contigs')."""
    return stage_table_text(TSV_HEADER, names, stages, lambda name, stage, length, r: _row(name, stage, length, r, peak), ZERO, totals)


def bed_text(k, peak, names, runs, min_run=1):
    """one line per run of at least min_run windows, seq and mate_seq indexing `names`:
    contig start end mate mate_start mate_end strand n_kmers read_copies deficit_fraction, the ends = start + n_kmers + k - 1,
    read_copies = sum_reads / (peak * n_kmers), deficit_fraction = n_deficit / n_kmers"""
    out = []
    for seq, start, nk, mate, mstart, strand, sr, nd in listed(runs, min_run):
        out.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\t%s\t%.4f\n" % (names[seq], start, start + nk + k - 1, names[mate], mstart, mstart + nk + k - 1, STRANDS[strand], nk,
                                                                  copies_text(sr, peak, nk), float(nd) / nk))
    return "".join(out)


def pairs(runs):
    """[(seq, mate_seq, strand, runs, windows, deficit, sum_reads)] over the runs of every length, ordered by seq, mate_seq, strand"""
    d = {}
    for seq, _, nk, mate, _, strand, sr, nd in listed(runs, 1):
        p = d.setdefault((seq, mate, strand), [0, 0, 0, 0])
        p[0] += 1
        p[1] += nk
        p[2] += nd
        p[3] += sr
    return [key + tuple(d[key]) for key in sorted(d)]


def pairs_tsv_text(peak, stages):
    """stages: [(stage name, names, runs)].  One row per (contig, mate, strand) with at least one run of any length, ordered by
    stage, contig order, mate order, strand (`+` first)"""
    out = [PAIRS_HEADER]
    for stage, names, runs in stages:
        for seq, mate, strand, nr, nw, nd, sr in pairs(runs):
            out.append("%s\t%s\t%s\t%s\t%d\t%d\t%d\t%s\n" % (stage, names[seq], names[mate], STRANDS[strand], nr, nw, nd, copies_text(sr, peak, nw)))
    return "".join(out)


def stage_log_text(rows, n_listed):
    """`N two-copy, M deficit, X multi and Y unplaced windows, R runs listed` of one stage"""
    t = totals(rows)
    return "%d two-copy, %d deficit, %d multi and %d unplaced windows, %d runs listed" % (t[2], t[3], t[4], t[5], n_listed)
