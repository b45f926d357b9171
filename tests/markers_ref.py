"""Marker sets and binning by two haplotype assemblies, restated in plain Python on top of readbins_ref: the select of
include/jasper_hip.h (jasper_table_select) and everything `python -m jasper_amd.triobin --hap1 .. --hap2 ..` writes.  Everything is driven
by dicts of canonical k-mer strings (-> count); nothing here is taken from the code under test.

Select.  A key x of `src` is a candidate when src[x] >= thre_src; a candidate is dropped as in_absent when absent holds it (count >= 1),
else as not_solid when `solid` is given and min(solid[x], 2^32-1) < thre_solid; what is left is selected and keeps its count in src.

Assembly mode.  hap1's and hap2's dicts come from their contigs (no k-mer spans two contigs), the child's from all read files.  markers
solid: M' = select(hap1, hap2, child, 1, thre_child), P' = select(hap2, hap1, child, 1, thre_child); markers all: no child.  M_total and
P_total are the numbers of keys of M' and P'; a read's counts are readbins_ref.read_counts against (M', P') with thresholds 1; the rule and
the two tables are readbins_ref's with the bins called hap1, hap2, unknown."""
import readbins_ref as ref

U32 = ref.U32
BINS = ("hap1", "hap2", "unknown")
_NAME = dict(zip(ref.BINS, BINS))


def select(src, absent, solid, thre_src, thre_solid):
    """-> ({key: count in src} of the selected keys, (candidates, in_absent, not_solid, selected))"""
    out, cand, in_absent, not_solid = {}, 0, 0, 0
    for x, c in src.items():
        if c < thre_src:
            continue
        cand += 1
        if absent.get(x, 0) != 0:
            in_absent += 1
        elif solid is not None and min(solid.get(x, 0), U32) < thre_solid:
            not_solid += 1
        else:
            out[x] = c
    return out, (cand, in_absent, not_solid, len(out))


def readbins_tsv(files, lens, ms, ps, bins):
    text = "#file\tbin\treads\tbases\thap1_markers\thap2_markers\n"
    tot = {b: [0, 0, 0, 0] for b in BINS}
    for f, fl, fm, fp, fb in zip(files, lens, ms, ps, bins):
        row = {b: [0, 0, 0, 0] for b in BINS}
        for ln, m, p, b in zip(fl, fm, fp, fb):
            for acc in (row[b], tot[b]):
                acc[0] += 1
                acc[1] += ln
                acc[2] += m
                acc[3] += p
        text += "".join("%s\t%s\t%d\t%d\t%d\t%d\n" % ((f, b) + tuple(row[b])) for b in BINS)
    return text + "".join("*\t%s\t%d\t%d\t%d\t%d\n" % ((b,) + tuple(tot[b])) for b in BINS)


def per_read_tsv(files, names, lens, ms, ps, bins):
    text = "#file\trecord\tname\tlength\thap1\thap2\tbin\n"
    for f, fn, fl, fm, fp, fb in zip(files, names, lens, ms, ps, bins):
        for i, (name, ln, m, p, b) in enumerate(zip(fn, fl, fm, fp, fb)):
            text += "%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % (f, i, name, ln, m, p, b)
    return text


class Haps:
    """the truth of one assembly-mode run: hap1 / hap2 = lists of contig sequences, reads = {input name: [(name, sequence)]} (all of
    them are the child's reads), markers "solid" (with thre_child) or "all" -> marker dicts, totals, the selects' counters, per input the
    per-read counts"""

    def __init__(self, k, hap1, hap2, reads, markers, thre_child=None):
        self.k, self.reads = k, reads
        d1, d2 = ref.kmer_dict(hap1, k), ref.kmer_dict(hap2, k)
        child = ref.kmer_dict([s for r in reads.values() for _, s in r], k) if markers == "solid" else None
        thre = thre_child if markers == "solid" else 1
        self.m, self.m_stats = select(d1, d2, child, 1, thre)
        self.p, self.p_stats = select(d2, d1, child, 1, thre)
        self.m_total, self.p_total = len(self.m), len(self.p)
        self.private = (self.m_stats[0] - self.m_stats[1], self.p_stats[0] - self.p_stats[1])      # before the solid filter
        self.counts = {f: ref.read_counts([s for _, s in r], k, self.m, self.p, 1, 1) for f, r in reads.items()}

    def files(self, paths, which, paired=False, min_markers=1):
        """paths: the inputs as given, which: the key of `reads` for each -> (readbins.tsv, reads.tsv, per input its bins)"""
        reads = [self.reads[w] for w in which]
        lens = [[len(s) for _, s in r] for r in reads]
        names = [[n for n, _ in r] for r in reads]
        ms, ps = [self.counts[w][0] for w in which], [self.counts[w][1] for w in which]
        bins = [[_NAME[b] for b in fb] for fb in ref.file_bins(ms, ps, self.m_total, self.p_total, min_markers, paired)]
        return readbins_tsv(paths, lens, ms, ps, bins), per_read_tsv(paths, names, lens, ms, ps, bins), bins


# ---- the fixture of the assembly-mode tests: the synthetic trio's two haplotypes as the assemblies, hap1 with assembly errors -----------
HAPS_THRE = 2


def with_errors(hap, first=700, every=1500):
    """a substitution at every `every`-th base from `first`: error i turns base c (its index in ACGT) into ACGT[(c + 1 + i % 3) % 4]"""
    b = bytearray(hap)
    for i, pos in enumerate(range(first, len(b), every)):
        b[pos] = b"ACGT"[(b"ACGT".index(bytes([b[pos]])) + 1 + i % 3) % 4]
    return bytes(b)


def make_haps():
    """-> dict(hap1, hap2 (one contig each), r1, r2): readbins_ref.make_trio's haplotypes and child reads, hap_a with errors"""
    t = ref.make_trio()
    return dict(hap1=with_errors(t["hap_a"]), hap2=t["hap_b"], r1=t["r1"], r2=t["r2"])


def histo_threshold(child):
    """the solid-k-mer rule on the reads' dict: the histogram (multiplicity -> distinct k-mers, non-zero rows in rising order) is followed
    downhill from its first row; the first row that RISES ends the descent, and the threshold is half the multiplicity (rounded down) of
    the descent's last row -> that threshold, or None when the histogram never rises or the threshold is below 2"""
    rows = {}
    for c in child.values():
        rows[min(c, 10001)] = rows.get(min(c, 10001), 0) + 1
    rows = sorted(rows.items())
    if not rows:
        return None
    floor_n, half = rows[0][1], 0
    for mult, n in rows[1:]:
        if n > floor_n:
            return half if half >= 2 else None
        floor_n, half = n, mult // 2
    return None


def noise_reads(seed=77):
    """reads of random sequence that give the fixture's histogram an error peak to descend from: 2000 k-mers once, 1000 twice, 300 three
    times (the trio's reads alone hold 76, 95, 3, 52, 133 k-mers 1 .. 5 times: no descent).  With them the rows fall from 1 to 4 and
    rise at 5, so the rule derives 4 // 2 = 2"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for i, (n, times) in enumerate(((2000, 1), (1000, 2), (300, 3))):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n + ref.TRIO_K - 1)].tobytes()
        out += [("noise%d.%d" % (i, j), s) for j in range(times)]
    return out


def fasta(name, seq, width=80):
    return b">" + name + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
