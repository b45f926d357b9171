"""Gap scan: the writers of `*.gaps.tsv`, `*.gaps*.bed`, `*.gapfills*.tsv` and the filled sequences (cli --gaps, kmerqc --gaps).

An extension: a Sealer-style closure.  A window that holds a non-base byte has no k-mer, so the `N` runs of a scaffolded assembly are
invisible to every other scan here; and the compound scan counts a run of unreliable k-mers that replaces more than 64 bytes as `long`
and stops.  The scan (KmerTable.gap_scan; semantics in include/jasper_hip.h, jasper_gap_scan) walks the solid k-mers of the reads from
the left flank of every such place -- the last solid window before it -- until they rejoin its right flank, for up to --gap-max-len
bases, and lists each string that does.  Unreliable k-mers that touch a gap (a dirty contig end) are part of its site and are replaced
with it, up to --gap-max-trim bases on either side.

Per contig the TSV counts the sites, the searched ones (not at a contig's edge, not ragged), the bridged ones (at least one record),
the unique ones (exactly one record and not complex), the records, and the sites that are at an edge, ragged (more than
--gap-max-trim unreliable bases between a flank and the gap), at the limit (strings were left at --gap-max-len) and complex (more than
64 strings of one length, or more than 16 records).

Limits: the walk is over exact k-mers of the reads, so a gap whose true sequence the reads do not cover with solid k-mers stays open; a
heterozygous difference inside a gap multiplies the front and gives two records (not unique); the closing rule ends a tandem expansion
at k - 1 bases; contig ends that overlap (a negative gap) are not joined; and only unique fills are applied (fill_sequences).

Nothing here touches the GPU: the functions take names, lengths, sequences, counters, sites and records.
"""
from .report import column_sums, stage_table_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\tsites\tsearched\tbridged\tunique\trecords\tedge\tragged\tlimit\tcomplex\n"
FILLS_HEADER = "#contig\tpos\tref_len\tlen\tref_min\talt_min\tfill\n"
ZERO = (0,) * 9
KINDS = {0: "explicit", 1: "gap", 2: "run"}
STATUS = {1: "dead", 2: "limit", 3: "complex", 4: "edge", 5: "ragged", 6: "skipped"}


def _row(name, stage, length, c):
    return "%s\t%s" % (name, stage) + "\t%d" * (1 + len(c)) % ((length,) + tuple(c)) + "\n"


def totals(counts):
    """column sums of the nine counters of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 9)


def gaps_tsv_text(names, stages):
    """stages: [(stage name, lengths, counts)], lengths[i] / counts[i] = contig i's length and nine counters, or None for a contig
    that stage does not have (a row of zeros).  Per contig in the order of `names` one row per stage, then one row per stage for
    contig `*` with the sums."""
    return stage_table_text(TSV_HEADER, names, stages, _row, ZERO, totals)


def site_fields(s):
    """(seq, a, q, kind, status, n_records, levels, trim_left, trim_right, ref_min) of an entry of GapScan.sites or of a tuple in the
    order of GapScan.site_tuples()"""
    if hasattr(s, "dtype"):
        return (int(s["seq"]), int(s["a"]), int(s["q"]), KINDS[int(s["kind"])], STATUS[int(s["status"])], int(s["n_records"]), int(s["levels"]),
                int(s["trim_left"]), int(s["trim_right"]), int(s["ref_min"]))
    return tuple(s)


def _text(y):
    return y if isinstance(y, str) else bytes(y).decode("latin-1")


def record_fields(r):
    """(seq, pos, ref_len, len, y, ref_min, alt_min) of a tuple in the order of GapScan.record_tuples()"""
    seq, pos, rlen, ln, y, rmin, amin = r
    return int(seq), int(pos), int(rlen), int(ln), _text(y), int(rmin), int(amin)


def is_unique(site):
    """exactly one record and not complex: the sites whose fill is applied"""
    return site[5] == 1 and site[4] != "complex"


def unique_fills(sites, records):
    """{(seq, a): record} of the unique sites"""
    keys = {(s[0], s[1]) for s in map(site_fields, sites) if is_unique(s)}
    return {(r[0], r[1]): r for r in map(record_fields, records) if (r[0], r[1]) in keys}


def bed_text(names, sites, records):
    """one line per site, in the order of the sites: contig a q kind status n_records trim_left trim_right fill_len alt_min; the last two
    are `.` unless the site is unique"""
    fills = unique_fills(sites, records)
    out = []
    for s in map(site_fields, sites):
        r = fills.get((s[0], s[1]))
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (names[s[0]], s[1], s[2], s[3], s[4], s[5], s[7], s[8], "." if r is None else "%d" % r[3],
                                                               "." if r is None else "%d" % r[6]))
    return "".join(out)


def fills_tsv_text(names, records):
    """one line per record, in the order of the records: contig pos ref_len len ref_min alt_min fill; fill is `.` for len 0"""
    out = [FILLS_HEADER]
    for seq, pos, rlen, ln, y, rmin, amin in map(record_fields, records):
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (names[seq], pos, rlen, ln, rmin, amin, y if ln else "."))
    return "".join(out)


def fill_sequences(seqs, sites, records):
    """the sequences with every unique site's s[a .. q) replaced by its y, in upper case; everything else stays byte for byte.  A
    sequence comes back as the type it came in (str or bytes)."""
    fills = unique_fills(sites, records)
    per_seq = {}
    for (seq, a), r in fills.items():
        per_seq.setdefault(seq, []).append((a, a + r[2], r[4]))
    out = []
    for i, s in enumerate(seqs):
        if i not in per_seq:
            out.append(s)
            continue
        parts, at = [], 0
        for a, q, y in sorted(per_seq[i]):
            parts.append(s[at:a])
            parts.append(y if isinstance(s, str) else y.encode("latin-1"))
            at = q
        parts.append(s[at:])
        out.append(("" if isinstance(s, str) else b"").join(parts))
    return out


def stage_log_text(counts):
    """`A sites, B searched, C bridged, D unique, E records, F edge, G ragged, H limit, I complex` of one stage"""
    return "%d sites, %d searched, %d bridged, %d unique, %d records, %d edge, %d ragged, %d limit, %d complex" % totals(counts)


def log_text(counts0, counts1):
    return "Gap scan: before polishing %s; after polishing %s" % (stage_log_text(counts0), stage_log_text(counts1))
