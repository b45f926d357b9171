"""Copy-number k-mer spectrum and completeness: the numbers derived from `KmerTable.spectrum` and the writers of
`*.spectra_cn*.tsv` and `*.completeness.tsv` (cli --spectra, kmerqc --spectra).

An extension: the reference has no counterpart.  The dense k-mer report (jasper_amd/report.py) reads in one direction only,
assembly windows against read counts; this is the other direction -- which share of the reads' solid k-mers the assembly holds
at all (completeness), how many distinct k-mers of every read multiplicity it holds 0, 1, 2, 3, 4 or more than 4 times
(spectra-cn: collapsed repeats, duplicated haplotigs, missing sequence), and how many distinct k-mers only the assembly has.

The spectrum is a matrix S of 6 rows (include/jasper_hip.h, jasper_table_spectrum): row m = min(copies in the assembly, 5),
column c = min(count in the reads, 10001); S[m][c] for c >= 1 counts distinct k-mers of the reads, S[m][0] for m >= 1 the
distinct k-mers that only the assembly has.

Nothing here touches the GPU: the functions take a KmerSpectrum, a numpy array or a list of rows.
"""
from .report import write_atomic  # noqa: F401  (every file of this module is written through it: `.tmp`, then renamed)

ROWS = 6
COLS = 10002
ROW_LABELS = ("0", "1", "2", "3", "4", ">4")
CN_HEADER = "#copies\tread_count\tkmers\n"
COMPLETENESS_HEADER = "#stage\tk\tthreshold\tsolid_kmers\tsolid_found\tcompleteness\tasm_distinct\tasm_only\n"


def cells_of(spec):
    """the matrix as a list of ROWS lists of Python ints (spec: KmerSpectrum, numpy array or list of rows)"""
    cells = getattr(spec, "cells", spec)
    rows = [[int(v) for v in row] for row in cells]
    if len(rows) != ROWS or any(len(r) != len(rows[0]) for r in rows) or not rows[0]:
        raise ValueError("a spectrum has %d rows of equal length" % ROWS)
    return rows


def derived(spec, threshold):
    """(solid, found, asm_distinct, asm_only) for a threshold t: solid = distinct k-mers of the reads with count >= t, found =
    those of them the assembly has, asm_distinct = distinct k-mers of the assembly, asm_only = those the reads do not have.
    A threshold below 1 counts as 1: a k-mer the reads do not have is never solid."""
    rows = cells_of(spec)
    t = max(1, int(threshold))
    solid = sum(sum(r[t:]) for r in rows)
    found = sum(sum(r[t:]) for r in rows[1:])
    asm_distinct = sum(sum(r) for r in rows[1:])
    asm_only = sum(r[0] for r in rows[1:])
    return solid, found, asm_distinct, asm_only


def completeness_pct(found, solid):
    """100 * found / solid, "%.4f"; "NA" when there is no solid k-mer"""
    if solid <= 0:
        return "NA"
    return "%.4f" % (100.0 * float(found) / float(solid))


def spectra_cn_text(spec):
    """header, then one row per non-zero cell ordered by (row, column): copies (0, 1, 2, 3, 4, >4), read_count (the column: 0 =
    only in the assembly, the last column = that count or more), kmers"""
    out = [CN_HEADER]
    for m, row in enumerate(cells_of(spec)):
        for c, v in enumerate(row):
            if v:
                out.append("%s\t%d\t%d\n" % (ROW_LABELS[m], c, v))
    return "".join(out)


def completeness_row(stage, spec, threshold):
    """(stage, threshold, solid, found, asm_distinct, asm_only): one row of completeness_text (the threshold as derived() applies it)"""
    return (stage, max(1, int(threshold))) + derived(spec, threshold)


def completeness_text(k, rows):
    """rows: [(stage, threshold, solid, found, asm_distinct, asm_only)] -> header and one line per row"""
    out = [COMPLETENESS_HEADER]
    for stage, thr, solid, found, asm_distinct, asm_only in rows:
        out.append("%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (stage, k, thr, solid, found, completeness_pct(found, solid), asm_distinct, asm_only))
    return "".join(out)


def log_text(row):
    """the log line of one completeness row (without its prefix)"""
    _, thr, solid, found, _, asm_only = row
    pct = completeness_pct(found, solid)
    return "k-mer completeness = %s (%d of %d solid k-mers, threshold %d); %d assembly-only k-mers" % (
        pct if pct == "NA" else pct + " %", found, solid, thr, asm_only)
