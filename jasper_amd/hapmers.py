"""Trio hap-mer evaluation: phase blocks and switch errors from the markers of a hap-mer scan, and the writers of `*.hapmers.tsv`,
`*.hapmers*.bed`, `*.phased_blocks*.bed` and `*.hapmer_completeness.tsv` (cli --hapmers, kmerqc --hapmers).

An extension: the reference has no counterpart.  The scan (KmerTable.hapmer_scan; semantics in include/jasper_hip.h,
jasper_hapmer_scan) says where a contig carries k-mers that only the mother's or only the father's reads hold; each maximal run of
such windows is one MARKER.  The census (KmerTable.hapmer_census) says how many such k-mers each parent has and how many of them the
assembly holds.  This module makes phase blocks of the markers: a polisher that moves a het site onto the other haplotype leaves
every other check of this project content, and shows here as a switch.

The block rule is this project's own (it is not Merqury's), stated in full in phase_blocks.

Nothing here touches the GPU: the functions take names, lengths, counters and runs.
"""
from .report import align, column_sums, contig_name, stage_table_text, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

TSV_HEADER = "#contig\tstage\tlength\twindows\tvalid\tmat\tpat\tmarkers\tblocks\tblock_n50\tswitch_markers\tswitch_kmers\tswitch_rate\n"
COMPLETENESS_HEADER = "#stage\thap\tk\tparent_threshold\tchild_threshold\thapmers\tfound\tcompleteness\toccurrences\n"
KINDS = {1: "mat", 2: "pat"}
ZERO = (0, 0, 0, 0)
SHORT_RANGE, MAX_SWITCHES = 20000, 100


def _run_fields(r):
    if hasattr(r, "dtype"):
        return tuple(int(r[f]) for f in ("seq", "start", "n_kmers", "kind"))
    return tuple(int(v) for v in r)


def markers_by_contig(runs, n_contigs):
    """the runs (seq, start, n_kmers, kind) of a scan as one list of markers (start, n_kmers, kind) per contig, in order"""
    out = [[] for _ in range(n_contigs)]
    for seq, start, nk, kind in (_run_fields(r) for r in runs):
        out[seq].append((start, nk, kind))
    return out


def _new_block(m):
    start, n, kind = m
    return {"start": start, "last": m, "kind": kind, "markers": 1, "kmers": n, "switch_markers": 0, "switch_kmers": 0}


def _own(block, m):
    block["markers"] += 1
    block["kmers"] += m[1]
    block["last"] = m


def phase_blocks(markers, k, short_range=SHORT_RANGE, max_switch_markers=MAX_SWITCHES):
    """markers: one contig's (start, n_kmers, kind) in order; a marker covers the windows [start, start + n_kmers).
    -> the contig's phase blocks, dicts of start, end, kind, markers, kmers, switch_markers, switch_kmers.

    A block starts with a marker and has that marker's kind.  A marker of the block's kind joins it.  Markers of the other kind are held
    back (`pend`): when the block's kind returns, they were SWITCHES inside the block -- counted, not part of its markers or k-mers.
    When more than max_switch_markers are held back, or they span more than short_range windows (the end of the last one minus the start
    of the first), the haplotype has changed for good: the block ends at its last own marker and the held-back markers start the next
    block, of their kind.  Markers still held back at the contig's end become a block of their own.
    start = the first own marker's start, end = the last own marker's start + n_kmers + k - 1 (the base after its last window)."""
    blocks, block, pend = [], None, []

    def emit(b):
        last = b.pop("last")
        b["end"] = last[0] + last[1] + k - 1
        blocks.append(b)

    for m in markers:
        if block is None:
            block = _new_block(m)
        elif m[2] == block["kind"]:
            block["switch_markers"] += len(pend)
            block["switch_kmers"] += sum(p[1] for p in pend)
            pend = []
            _own(block, m)
        else:
            pend.append(m)
            if len(pend) > max_switch_markers or (m[0] + m[1]) - pend[0][0] > short_range:
                emit(block)
                block = _new_block(pend[0])
                for p in pend[1:]:
                    _own(block, p)
                pend = []
    if block is not None:
        emit(block)
    if pend:
        block = _new_block(pend[0])
        for p in pend[1:]:
            _own(block, p)
        emit(block)
    return blocks


def block_n50(blocks):
    """over the blocks' lengths end - start: the largest L such that the blocks of length >= L hold at least half of the summed
    length; 0 without blocks"""
    lens = sorted((b["end"] - b["start"] for b in blocks), reverse=True)
    total, acc = sum(lens), 0
    for ln in lens:
        acc += ln
        if 2 * acc >= total:
            return ln
    return 0


def switch_rate_text(n_markers, kmers, switch_kmers):
    """100 * switch_kmers / (kmers + switch_kmers), "%.4f"; "NA" for a contig without a marker"""
    if n_markers <= 0 or kmers + switch_kmers <= 0:
        return "NA"
    return "%.4f" % (100.0 * switch_kmers / (kmers + switch_kmers))


def contig_stats(n_markers, blocks):
    """(markers, blocks, block_n50, switch_markers, switch_kmers, own k-mers of the blocks)"""
    return (n_markers, len(blocks), block_n50(blocks), sum(b["switch_markers"] for b in blocks), sum(b["switch_kmers"] for b in blocks), sum(b["kmers"] for b in blocks))


class Stage:
    """one scan made into what the files need: per contig the counters, the markers and the phase blocks"""

    def __init__(self, k, names, lengths, counts, runs, short_range=SHORT_RANGE, max_switch_markers=MAX_SWITCHES):
        self.k, self.names, self.lengths, self.counts, self.runs = k, list(names), list(lengths), list(counts), runs
        self.markers = markers_by_contig(runs, len(self.names))
        self.blocks = [phase_blocks(m, k, short_range, max_switch_markers) for m in self.markers]

    def aligned(self, names):
        """(lengths, counts, markers, blocks) in the order of `names`, None where this stage lacks a contig (report.align's rule)"""
        idx = list(range(len(self.names)))
        lengths, where = align(names, self.names, self.lengths, idx)
        pick = lambda xs: [None if j is None else xs[j] for j in where]
        return lengths, pick(self.counts), pick(self.markers), pick(self.blocks)

    def all_blocks(self):
        return [b for bs in self.blocks for b in bs]


def totals(counts):
    """column sums of the (windows, valid, mat, pat) of the contigs that have any (None = contig missing)"""
    return column_sums(counts, 4)


def _row(name, stage, length, r):
    (w, v, m, p), markers, blocks = r
    nm, nb, n50, sm, sk, own = contig_stats(len(markers), blocks)
    return "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, stage, length, w, v, m, p, nm, nb, n50, sm, sk, switch_rate_text(nm, own, sk))


def hapmers_tsv_text(names, stages):
    """stages: [(stage name, Stage)].  Per contig in the order of `names` one row per stage (zeros and NA for a contig that stage does
    not have), then one row per stage for contig `*`: the sums, the N50 over all blocks and the switch rate over all of them."""
    rows = []                                    # a contig's row: (counts, markers, blocks)
    for stage, s in stages:
        lengths, counts, markers, blocks = s.aligned(names)
        rows.append((stage, lengths, [None if c is None else (c, markers[i], blocks[i]) for i, c in enumerate(counts)]))
    return stage_table_text(TSV_HEADER, names, rows, _row, (ZERO, [], []),
                            lambda rs: (totals([r and r[0] for r in rs]), [m for r in rs if r for m in r[1]], [b for r in rs if r for b in r[2]]))


def bed_text(k, names, runs):
    """one line per marker, seq indexing `names`: contig start end hap n_kmers, end = start + n_kmers + k - 1, hap = mat / pat"""
    return "".join("%s\t%d\t%d\t%s\t%d\n" % (names[seq], start, start + nk + k - 1, KINDS[kind], nk) for seq, start, nk, kind in (_run_fields(r) for r in runs))


def blocks_bed_text(names, blocks_per_contig):
    """one line per phase block: contig start end hap markers kmers switch_markers switch_kmers"""
    out = []
    for name, blocks in zip(names, blocks_per_contig):
        for b in blocks:
            out.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (name, b["start"], b["end"], KINDS[b["kind"]], b["markers"], b["kmers"], b["switch_markers"], b["switch_kmers"]))
    return "".join(out)


def completeness_value_text(found, hapmers):
    return "NA" if hapmers <= 0 else "%.4f" % (100.0 * found / hapmers)


def completeness_text(k, thre_mat, thre_pat, thre_child, stages):
    """stages: [(stage name, census)], census with .mat / .pat = (hapmers, found, occurrences): two rows (mat, pat) per stage"""
    out = [COMPLETENESS_HEADER]
    for stage, cen in stages:
        for hap, thre, (h, f, occ) in (("mat", thre_mat, cen.mat), ("pat", thre_pat, cen.pat)):
            out.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (stage, hap, k, thre, thre_child, h, f, completeness_value_text(f, h), occ))
    return "".join(out)


def stage_log_text(stage, census):
    """`M mat and P pat windows in R markers, B blocks (N50 L), switch rate S %; completeness mat X pat Y` of one stage"""
    t = totals(stage.counts)
    blocks = stage.all_blocks()
    nm, nb, n50, _, sk, own = contig_stats(len(stage.runs), blocks)
    return "%d mat and %d pat windows in %d markers, %d blocks (N50 %d), switch rate %s; hap-mer completeness mat %s pat %s" % (
        t[2], t[3], nm, nb, n50, switch_rate_text(nm, own, sk), completeness_value_text(census.mat[1], census.mat[0]), completeness_value_text(census.pat[1], census.pat[0]))
