"""Writers of the dense k-mer report: `$QUERY_FN.kmer_qv.tsv` and `$QUERY_FN.unreliable.*.bed` (cli --report, kmerqc).

An extension: the reference prints two Q values for the whole assembly (src/jasper.sh:239-242) from a strided walk over chunk
records (src/jasper.py:50-111).  The files written here come from the DENSE scan of whole contigs (KmerTable.kmer_report:
every window, also those that span two chunk records), so their totals differ from the reference's (bad, total) -- on
tests/golden/cases/cluster_k25 the walk says 443 bad of 5976, the dense scan 450 unreliable of 5976 valid: the walk jumps k-2
windows after a good one and never sees a k-mer across a chunk boundary.

Nothing here touches the GPU: the functions take names, lengths, counters and runs.
"""
import math
import os

TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\tunreliable\tabsent\tQV_unreliable\tQV_absent\n"


def qv_text(x, valid, k):
    """-10 log10(1 - (1 - x/valid)^(1/k)) (the formula of src/jasper.sh:239-242 on dense counters), "%.4f"; "inf" when no
    window is counted against the sequence, "NA" when it has no valid window"""
    if valid <= 0:
        return "NA"
    if x <= 0:
        return "inf"
    p = 1.0 - (1.0 - float(x) / float(valid)) ** (1.0 / k)
    return "%.4f" % (-10.0 * math.log10(p) + 0.0)


def contig_name(header):
    """first whitespace token of a header line, without its '>'"""
    tok = header.split()[0] if header.split() else ""
    return tok[1:] if tok.startswith(">") else tok


def _row(name, stage, length, c, k):
    w, v, u, a = c
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name, stage, length, w, v, u, a, qv_text(u, v, k), qv_text(a, v, k))


def column_sums(rows, width):
    """the sums of the first `width` columns over the contigs that have a row (None = contig missing)"""
    return tuple(sum(r[i] for r in rows if r is not None) for i in range(width))


def stage_table_text(header, names, stages, row, zero, sums):
    """the table that every scan writes.  stages: [(stage name, lengths, rows)], lengths[i] / rows[i] = contig i's length and counters,
    or None for a contig that stage does not have (length 0 and the row `zero`).  Per contig in the order of `names` one line per
    stage, then one line per stage for contig `*` with sums(rows); row(name, stage, length, r) makes a line."""
    out = [header]
    for i, name in enumerate(names):
        for stage, lengths, rows in stages:
            r = rows[i]
            out.append(row(name, stage, lengths[i] if r is not None else 0, r if r is not None else zero))
    for stage, lengths, rows in stages:
        out.append(row("*", stage, sum(ln for ln, r in zip(lengths, rows) if r is not None), sums(rows)))
    return "".join(out)


def vcf_preamble(source, names, lengths, infos):
    """the lines of a VCFv4.2 file before its records: `##source=jasper_amd <source>`, one `##contig` line per contig in the order of
    `names`, one `##INFO` line per (ID, Type, Description) of `infos` (Number=1 each) and the column line"""
    out = ["##fileformat=VCFv4.2\n", "##source=jasper_amd %s\n" % source]
    out += ["##contig=<ID=%s,length=%d>\n" % (name, ln) for name, ln in zip(names, lengths)]
    out += ['##INFO=<ID=%s,Number=1,Type=%s,Description="%s">\n' % info for info in infos]
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    return out


def totals(counts):
    """column sums of the (windows, valid, unreliable, absent) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 4)


def qv_tsv_text(k, names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and (windows, valid, unreliable,
    absent), or None for a contig that stage does not have (a row of zeros and NA).  Per contig in the order of `names` one row
    per stage, then one row per stage for contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, lambda name, stage, length, c: _row(name, stage, length, c, k), (0, 0, 0, 0), totals)


def bed_text(k, names, runs):
    """one line per run (seq, start, n_kmers, n_absent, min_count), seq indexing `names`:
    contig start end n_kmers n_absent min_count core_start core_end, end = start + n_kmers + k - 1; the core = the bases that
    every window of the run covers, [start + n_kmers - 1, start + k) when n_kmers <= k, else empty (core_start = core_end = start)"""
    out = []
    for r in runs:
        seq, start, nk, na, mn = (int(r[f]) for f in ("seq", "start", "n_kmers", "n_absent", "min_count")) if hasattr(r, "dtype") else (int(v) for v in r)
        if nk <= k:
            cs, ce = start + nk - 1, start + k
        else:
            cs = ce = start
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (names[seq], start, start + nk + k - 1, nk, na, mn, cs, ce))
    return "".join(out)


def write_atomic(path, text):
    with open(path + ".tmp", "w") as f:
        f.write(text)
    os.replace(path + ".tmp", path)


def align(names, other_names, other_lengths, other_counts):
    """the counters of a second set of contigs (the polished FASTA) in the order of `names`; a name that occurs several times
    is matched in order; None where the second set has no such contig"""
    where = {}
    for j, n in enumerate(other_names):
        where.setdefault(n, []).append(j)
    lengths, counts = [], []
    for n in names:
        js = where.get(n)
        if js:
            j = js.pop(0)
            lengths.append(other_lengths[j])
            counts.append(other_counts[j])
        else:
            lengths.append(0)
            counts.append(None)
    return lengths, counts

