"""The trio read binning restated in plain Python: the per-read counts of include/jasper_hip.h (jasper_read_bins), the binning rule of
README.md and the two tables `python -m jasper_amd.triobin` writes.  Everything is driven by dicts of canonical k-mer strings (bytes ->
count); nothing here is taken from the code under test.

Counts.  Read i of a packed text is text[offsets[i] : offsets[i+1]].  A window is k consecutive bytes of ONE read; it is valid iff all of
them are ACGTacgt; m, p = the counts of its case-folded canonical k-mer in the mother's and the father's dict, clamped to 2^32-1.
mat[i] = the valid windows of read i with m >= thre_mat and p == 0, pat[i] = those with p >= thre_pat and m == 0.

Rule.  A template's m and p are its read's counts (with pairs: the sums over its two mates).  m + p < min_markers -> unknown; else
m * P_total > p * M_total -> mat; else m * P_total < p * M_total -> pat; else unknown.  Python integers: exact at any size."""
U32 = 2**32 - 1
BINS = ("mat", "pat", "unknown")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_BASES = frozenset(b"ACGTacgt")


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def canonical(kmer):
    rc = kmer.translate(_COMP)[::-1]
    return kmer if kmer < rc else rc


def window_keys(read, k):
    """per window of one read: None (not valid) or its canonical k-mer"""
    b = as_bytes(read)
    out = []
    for i in range(len(b) - k + 1):
        w = b[i:i + k]
        out.append(canonical(w.upper()) if all(c in _BASES for c in w) else None)
    return out


def kmer_dict(seqs, k, times=1):
    """canonical k-mer -> occurrences over the sequences' valid windows, each taken `times` times"""
    d = {}
    for s in seqs:
        for key in window_keys(s, k):
            if key is not None:
                d[key] = d.get(key, 0) + times
    return d


def split(text, offsets):
    t = as_bytes(text)
    return [t[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def pack(reads):
    """reads -> (text, offsets)"""
    bs = [as_bytes(r) for r in reads]
    offs = [0]
    for b in bs:
        offs.append(offs[-1] + len(b))
    return b"".join(bs), offs


def read_counts(reads, k, md, pd, thre_mat, thre_pat):
    """(mat, pat): two lists, one entry per read"""
    mat, pat = [], []
    for r in reads:
        nm = np_ = 0
        for key in window_keys(r, k):
            if key is None:
                continue
            m, p = min(md.get(key, 0), U32), min(pd.get(key, 0), U32)
            nm += m >= thre_mat and p == 0
            np_ += p >= thre_pat and m == 0
        mat.append(nm)
        pat.append(np_)
    return mat, pat


def hapmer_total(own, other, thre):
    """a parent's number of hap-mers: its keys with count >= thre that the other parent does not hold"""
    return sum(1 for x, c in own.items() if min(c, U32) >= thre and other.get(x, 0) == 0)


def bin_of(m, p, m_total, p_total, min_markers=1):
    if m + p < min_markers:
        return "unknown"
    a, b = m * p_total, p * m_total
    return "mat" if a > b else "pat" if a < b else "unknown"


def file_bins(ms, ps, m_total, p_total, min_markers=1, paired=False):
    """ms / ps: per input file the per-read counts -> per input file the per-read bins.  paired: files 2j and 2j+1 are R1 and R2, record
    i of both is one template, decided by the sums"""
    out = []
    if not paired:
        for fm, fp in zip(ms, ps):
            out.append([bin_of(m, p, m_total, p_total, min_markers) for m, p in zip(fm, fp)])
        return out
    for j in range(0, len(ms), 2):
        assert len(ms[j]) == len(ms[j + 1])
        b = [bin_of(m1 + m2, p1 + p2, m_total, p_total, min_markers) for m1, m2, p1, p2 in zip(ms[j], ms[j + 1], ps[j], ps[j + 1])]
        out += [b, list(b)]
    return out


def readbins_tsv(files, lens, ms, ps, bins):
    """PREFIX.readbins.tsv: per file three rows (mat, pat, unknown), then file `*`; the marker columns sum each read's OWN counts"""
    text = "#file\tbin\treads\tbases\tmat_markers\tpat_markers\n"
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
    """PREFIX.readbins.reads.tsv: one line per read in input order, `record` 0-based within its file"""
    text = "#file\trecord\tname\tlength\tmat\tpat\tbin\n"
    for f, fn, fl, fm, fp, fb in zip(files, names, lens, ms, ps, bins):
        for i, (name, ln, m, p, b) in enumerate(zip(fn, fl, fm, fp, fb)):
            text += "%s\t%d\t%s\t%d\t%d\t%d\t%s\n" % (f, i, name, ln, m, p, b)
    return text


# ---- the synthetic trio of the CLI test (and of the host test that shows it is no vacuous input) ------------------------------------
TRIO_K = 21


def revcomp(s):
    return as_bytes(s).translate(_COMP)[::-1]


def make_trio(seed=2024, length=20000, stretch=(9000, 11000), read_len=150, step=13):
    """two haplotypes of one random genome of `length` bases: each carries its own SNPs, one about every 100 bases (at 100 i + 50 +- 20,
    the two haplotypes' at different places), none inside `stretch` and one on either side of it.  The mother is haplotype A and the father haplotype B, each at depth 4:
    four records of the whole haplotype.  The child's templates are pairs of `read_len`-base reads drawn from both haplotypes in turn, R1
    forward from every step-th position and R2 the reverse complement of the read 200 bases further on; a few carry N, lower case, are
    shorter than k or empty.  -> dict(hap_a, hap_b, r1, r2) with r1 / r2 = [(name, sequence)]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)]
    haps = []
    for h in range(2):
        g = genome.copy()
        places = [100 * i + 50 + int(rng.integers(-20, 21)) + (0 if h == 0 else 7) for i in range(length // 100)] + [stretch[0] - 1, stretch[1]]
        for pos in places:
            if stretch[0] <= pos < stretch[1] or pos >= length:
                continue
            g[pos] = b"ACGT"[(b"ACGT".index(bytes([g[pos]])) + int(rng.integers(1, 4))) % 4]
        haps.append(g.tobytes())
    r1, r2 = [], []
    for n, start in enumerate(range(0, length - read_len - 200, step)):
        hap = haps[n % 2]
        a, b = bytearray(hap[start:start + read_len]), bytearray(revcomp(hap[start + 200:start + 200 + read_len]))
        if n % 389 == 5:
            a[40] = ord("N")
        if n % 389 == 6:
            b[60:90] = bytes(b[60:90]).lower()
        if n % 389 == 7:
            a = a[:TRIO_K - 1]
        if n % 389 == 8:
            b = bytearray()
        r1.append(("t%d/1" % n, bytes(a)))
        r2.append(("t%d/2" % n, bytes(b)))
    return dict(hap_a=haps[0], hap_b=haps[1], r1=r1, r2=r2)


def fastq_text(reads, eol=b"\n"):
    return b"".join(b"@" + name.encode() + b" len=%d" % len(s) + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for name, s in reads)


def parent_fasta(hap, depth=4, width=80):
    lines = b"".join(hap[i:i + width] + b"\n" for i in range(0, len(hap), width))
    return b"".join(b">copy%d\n" % d + lines for d in range(depth))
