"""GPU: the trio read binning kernel (KmerTable.read_bins / read_bins_device, jasper_read_bins) against the restatement of its semantics
in tests/readbins_ref.py, exactly.  Nothing expected here comes from the code under test; the restatement itself is checked by hand in
test_triobin_host.py.

What the kernel can get wrong is where reads begin: its work is cut over the packed text (a thread owns 16 bytes, a workgroup a tile of
4096 windows), so the shapes here put read starts on every offset of a 16-byte group, on both sides of every tile seam, several into one
group, and let many threads add to one read's counters."""
import numpy as np
import pytest

import readbins_ref as ref

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
TILE = 4096
DEPTH, THRE = 3, 2
KS = [19, 41, 63]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    return KmerTable


def rand_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def table(KT, k, text, min_slots=1 << 16):
    t = KT(k, min_slots=min_slots)
    t.count_bases(bytes(text))
    return t


class Parents:
    """two haplotypes of one random genome with a SNP about every 100 bases each, as the mother's and the father's table at depth DEPTH,
    and the same as dicts.  `child` is a mosaic of the two: what the reads are cut from."""

    def __init__(self, KT, k, n, seed):
        rng = np.random.default_rng(seed)
        genome = bytearray(rand_seq(rng, n))
        self.k, self.haps = k, []
        for _ in range(2):
            h = bytearray(genome)
            for pos in range(50, n, 100):
                p = min(pos + int(rng.integers(-30, 31)), n - 1)
                h[p] = b"ACGT"[(b"ACGT".index(h[p]) + int(rng.integers(1, 4))) % 4]
            self.haps.append(bytes(h))
        a, b = self.haps
        self.child = b"".join((a if (i // 700) % 2 == 0 else b)[i:i + 700] for i in range(0, n, 700))
        self.md, self.pd = ref.kmer_dict([a], k, DEPTH), ref.kmer_dict([b], k, DEPTH)
        self.M, self.P = table(KT, k, b"N".join([a] * DEPTH)), table(KT, k, b"N".join([b] * DEPTH))

    def want(self, reads, tm=THRE, tp=THRE):
        return ref.read_counts(reads, self.k, self.md, self.pd, tm, tp)

    def close(self):
        self.M.close()
        self.P.close()


@pytest.fixture(scope="module")
def parents(KT):
    made = {k: Parents(KT, k, 3 * TILE + 2 * k + 600, 4000 + k) for k in KS}
    yield made
    for p in made.values():
        p.close()


def check(res, want, what):
    assert res.mat.dtype == np.uint32 and res.pat.dtype == np.uint32
    assert res.mat.tolist() == want[0], what
    assert res.pat.tolist() == want[1], what


def cut(text, lengths, forced=()):
    """text cut into reads of the lengths given, cycled, and once more at every position of `forced`"""
    reads, at, i, forced = [], 0, 0, sorted(set(forced))
    while at < len(text):
        end = min(at + lengths[i % len(lengths)], len(text))
        nxt = [f for f in forced if at < f < end]
        end = nxt[0] if nxt else end
        reads.append(text[at:end])
        at, i = end, i + 1
    return reads


def starts_of(reads):
    return set(np.cumsum([0] + [len(r) for r in reads])[:-1].tolist())


@pytest.mark.parametrize("k", KS)
def test_seams(KT, parents, k):
    """at least three tiles of packed text; read lengths cycle through 0, 0, 1, k-1, k, k+1, 15, 16, 17, 150, 151, and a read begins right
    before, at and right after the byte where each tile's first window ends and where it begins"""
    t = parents[k]
    text = t.child
    assert len(text) - k + 1 > 3 * TILE
    seams = [x for s in range(TILE, len(text), TILE) for x in (s - 1, s, s + 1, s + k - 2, s + k - 1, s + k)]
    reads = cut(text, [0, 0, 1, k - 1, k, k + 1, 15, 16, 17, 150, 151], seams)
    starts = starts_of(reads)
    assert b"".join(reads) == text and set(seams) <= starts and {s % 16 for s in starts} == set(range(16))
    assert reads.count(b"") > 50
    want = t.want(reads)
    assert sum(want[0]) > 100 and sum(want[1]) > 100 and sum(1 for m, p in zip(*want) if m and p) >= 1
    check(KT.read_bins(t.M, t.P, reads, THRE, THRE), want, "seams k=%d" % k)
    # the same text shifted through a 16-byte group by a first read of 1 .. 15 bytes (shorter than k: it has no window)
    for shift in (1, 7, 15):
        shifted = [b"ACGTACGTACGTACGT"[:shift]] + reads
        check(KT.read_bins(t.M, t.P, shifted, THRE, THRE), ([0] + want[0], [0] + want[1]), "seams k=%d shift %d" % (k, shift))


@pytest.mark.parametrize("k", KS)
def test_split_marker(KT, k):
    """a marker k-mer cut between read i and read i+1 at every cut point gives 0 in both; uncut inside one read it gives 1"""
    rng = np.random.default_rng(100 + k)
    x, y = rand_seq(rng, k), rand_seq(rng, k)
    M, P = table(KT, k, x), table(KT, k, y)
    md, pd = ref.kmer_dict([x], k), ref.kmer_dict([y], k)
    pre, post = rand_seq(rng, 23), rand_seq(rng, 29)
    reads = []
    for c in range(1, k):
        reads += [pre + x[:c], x[c:] + post]
    reads += [pre + x + post, pre + ref.revcomp(y) + post]
    want = ref.read_counts(reads, k, md, pd, 1, 1)
    assert want == ([0] * (2 * k - 2) + [1, 0], [0] * (2 * k - 2) + [0, 1])
    check(KT.read_bins(M, P, reads, 1, 1), want, "split marker k=%d" % k)
    M.close()
    P.close()


@pytest.mark.parametrize("k", [19, 63])
def test_many_adders_on_one_read(KT, k):
    """one read of 3 x 4096 + k bases whose every window is a maternal marker -- every thread of three tiles adds to one counter -- with a
    row of tiny reads before and after it"""
    rng = np.random.default_rng(200 + k)
    big = rand_seq(rng, 3 * TILE + k)
    other = rand_seq(rng, 500)
    M, P = table(KT, k, big), table(KT, k, other)
    md, pd = ref.kmer_dict([big], k), ref.kmer_dict([other], k)
    tiny = [rand_seq(rng, n % 7) for n in range(45)]
    reads = tiny + [big] + tiny
    want = ref.read_counts(reads, k, md, pd, 1, 1)
    assert want[0][45] == len(big) - k + 1 == 3 * TILE + 1 and sum(want[0]) == want[0][45] and sum(want[1]) == 0
    check(KT.read_bins(M, P, reads, 1, 1), want, "many adders k=%d" % k)
    M.close()
    P.close()


def test_dense_boundaries(KT, parents):
    """several thousand reads of exactly k bases (one window each), then several thousand shorter than 16: some 16-byte groups hold more
    than one start"""
    k = 19
    t = parents[k]
    text = t.child * 7
    whole = [text[i:i + k] for i in range(0, 3000 * k, k)]
    short = cut(text[3000 * k:], [3, 0, 15, 1, 7, 2, 0, 0, 11, 5, 14, 4])[:4000]
    reads = whole + short
    assert len(whole) == 3000 and len(short) == 4000 and max(len(r) for r in short) < 16
    want = t.want(reads)
    assert 300 < sum(want[0]) + sum(want[1]) <= 3000 and max(want[0] + want[1]) == 1 and sum(want[0][3000:]) + sum(want[1][3000:]) == 0
    check(KT.read_bins(t.M, t.P, reads, THRE, THRE), want, "dense boundaries")


@pytest.mark.parametrize("k", KS)
def test_bytes(KT, parents, k):
    """N and other non-base bytes and lower case inside reads; a read that is all N"""
    t = parents[k]
    rng = np.random.default_rng(300 + k)
    reads = []
    for i, start in enumerate(range(0, 6000, 150)):
        r = bytearray(t.child[start:start + 150 + i % 3])
        if i % 4 == 0:
            r[int(rng.integers(0, len(r)))] = ord("N")
        if i % 4 == 1:
            for bad in (b"n", b"-", b"\x00", b"\xff", b"*", b"U", b"@"):
                r[int(rng.integers(0, len(r)))] = bad[0]
        if i % 4 == 2:
            a = int(rng.integers(0, 100))
            r[a:a + 45] = bytes(r[a:a + 45]).lower()
        reads.append(bytes(r))
    reads += [b"N" * 200, t.child[100:300].lower(), b"N" + t.child[300:300 + k] + b"N", b"N" * 16 + t.child[400:400 + k - 1] + b"N" * 16]
    want = t.want(reads)
    assert sum(want[0]) > 20 and sum(want[1]) > 20 and want[0][-4] == want[1][-4] == 0
    check(KT.read_bins(t.M, t.P, reads, THRE, THRE), want, "bytes k=%d" % k)


@pytest.mark.parametrize("k", [19, 41])
def test_thresholds(KT, k):
    """a k-mer with count thre - 1 in a parent is no marker; a k-mer with count 1 in the other parent kills a marker; a count above 2^32
    still qualifies, at a threshold of 2^32 - 1 too; the same for both parents"""
    import layout_util as lu
    rng = np.random.default_rng(400 + k)
    thre, big = 3, 2**33 + 5
    both = rand_seq(rng, k)
    keys, dicts, tabs = [], [], []
    for side in range(2):
        below, killed, huge, plain = (rand_seq(rng, k) for _ in range(4))
        keys.append((below, killed, huge, plain))
        dicts.append({below: thre - 1, killed: thre, plain: thre, both: thre})
    for side in range(2):
        counts = dict(dicts[side])
        counts[keys[1 - side][1]] = 1                   # ... and the other parent's `killed` once
        tab = KT(k, min_slots=1 << 16)
        tab.count_bases(b"N".join((x if i % 2 else ref.revcomp(x)) for x, c in counts.items() for i in range(c)))
        tab.import_entries(lu.entries([lu.hash_of_kmer(keys[side][2].decode())], [big]))
        counts[keys[side][2]] = big
        tabs.append(tab)
        dicts[side] = {ref.canonical(x): c for x, c in counts.items()}
    (M, P), (md, pd) = tabs, dicts
    flank = rand_seq(rng, 40)
    reads = [flank + x + flank for side in keys for x in side] + [flank + both, keys[0][2] + flank + keys[1][3] + keys[0][0] + ref.revcomp(keys[0][3])]
    want = ref.read_counts(reads, k, md, pd, thre, thre)
    assert want == ([0, 0, 1, 1, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 0, 1, 1, 0, 1])
    check(KT.read_bins(M, P, reads, thre, thre), want, "thresholds k=%d" % k)
    for tm, tp in ((thre - 1, thre + 1), (U32, 1), (1, U32)):
        check(KT.read_bins(M, P, reads, tm, tp), ref.read_counts(reads, k, md, pd, tm, tp), "thresholds k=%d at %d, %d" % (k, tm, tp))
    assert ref.read_counts(reads, k, md, pd, U32, U32) == ([0, 0, 1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1, 0, 0, 0])      # only the counts above 2^32
    M.close()
    P.close()


def test_entry_points(KT, parents):
    import torch
    t = parents[41]
    reads = cut(t.child[:5000], [150, 0, 151, 40, 41, 149])
    want = t.want(reads)
    assert sum(want[0]) > 10 and sum(want[1]) > 10
    before = t.M.histogram(), t.P.histogram()
    first = KT.read_bins(t.M, t.P, reads, THRE, THRE)
    check(first, want, "list")
    assert first.seconds > 0
    text, offs = ref.pack(reads)
    offs = np.array(offs, dtype=np.int64)
    assert KT.read_bins(t.M, t.P, (text, offs), THRE, THRE) == first
    assert KT.read_bins(t.M, t.P, (np.frombuffer(text, dtype=np.uint8), offs.tolist()), THRE, THRE) == first
    assert KT.read_bins(t.M, t.P, [r.decode("latin-1") for r in reads], THRE, THRE) == first
    # offsets[0] > 0: what lies before the first read and after the last is not read, though it is full of markers
    junk = t.child[5000:5300]
    assert KT.read_bins(t.M, t.P, (junk + text + junk, offs + len(junk)), THRE, THRE) == first
    # the text in HBM, its pointer moved through a 16-byte group
    for shift in range(16):
        d = torch.frombuffer(bytearray(b"\x00" * shift + junk + text + junk), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert KT.read_bins_device(t.M, t.P, d.data_ptr() + shift, offs + len(junk), THRE, THRE) == first, shift
    d = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert KT.read_bins_device(t.M, t.P, d, offs, THRE, THRE) == first
    # no reads; reads without a window; two calls in a row
    for empty in (KT.read_bins(t.M, t.P, [], THRE, THRE), KT.read_bins(t.M, t.P, (b"ACGT", [2]), THRE, THRE), KT.read_bins_device(t.M, t.P, 0, [0], THRE, THRE)):
        assert len(empty.mat) == 0 and len(empty.pat) == 0
    check(KT.read_bins(t.M, t.P, [b"", b"", t.child[:40], b""], THRE, THRE), ([0] * 4, [0] * 4), "no window")
    assert KT.read_bins(t.M, t.P, reads, THRE, THRE) == first
    assert (t.M.histogram(), t.P.histogram()) == before


def test_against_the_hapmer_scan(KT, parents):
    """on a few hundred random reads mat / pat equal counters 2 and 3 of the hap-mer scan without a child table: the kernel a user could
    call before this one, one sequence per read"""
    t = parents[19]
    rng = np.random.default_rng(77)
    reads = []
    for _ in range(300):
        a, n = int(rng.integers(0, len(t.child) - 200)), int(rng.integers(0, 200))
        r = bytearray(t.child[a:a + n])
        if n and rng.integers(0, 5) == 0:
            r[int(rng.integers(0, n))] = ord("N")
        reads.append(bytes(r))
    scan = KT.hapmer_scan_parents(t.M, t.P, reads, THRE, THRE)
    res = KT.read_bins(t.M, t.P, reads, THRE, THRE)
    assert res.mat.tolist() == [c[2] for c in scan.counts] and res.pat.tolist() == [c[3] for c in scan.counts]
    assert sum(res.mat.tolist()) > 100 and sum(res.pat.tolist()) > 100
    check(res, t.want(reads), "random reads")


def test_refusals(KT, parents):
    """every cause of include/jasper_hip.h that one GPU can make gives an error return with its message, not a crash"""
    from test_gpu_shard import make_shards
    t = parents[19]
    reads = [t.child[:300], t.child[300:450]]
    other = table(KT, 27, t.child[:2000])
    with pytest.raises(Exception, match="different k"):
        KT.read_bins(t.M, other, reads, THRE, THRE)
    with pytest.raises(Exception, match="different k"):
        KT.read_bins(other, t.P, reads, THRE, THRE)
    other.close()
    shards, _ = make_shards(KT, t.M, 2, t.M.info()["slots"])
    for o, s in enumerate(shards):
        s.attach_tables(shards, o)
    with pytest.raises(Exception, match="maternal table must be a whole table"):
        KT.read_bins(shards[0], t.P, reads, THRE, THRE)
    with pytest.raises(Exception, match="paternal table must be a whole table"):
        KT.read_bins(t.M, shards[1], reads, THRE, THRE)
    for s in shards:
        s.close()
    with pytest.raises(Exception, match="the same table"):
        KT.read_bins(t.M, t.M, reads, THRE, THRE)
    for bad, who in (((0, THRE), "maternal"), ((THRE, 0), "paternal")):
        with pytest.raises(Exception, match="%s threshold must be at least 1" % who):
            KT.read_bins(t.M, t.P, reads, *bad)
    text = b"".join(reads)
    with pytest.raises(Exception, match="offsets must not decrease"):
        KT.read_bins(t.M, t.P, (text, [0, 300, 200]), THRE, THRE)
    with pytest.raises(Exception, match="null text"):
        KT.read_bins_device(t.M, t.P, 0, [0, 300], THRE, THRE)
    with pytest.raises(ValueError, match="outside the buffer"):
        KT.read_bins(t.M, t.P, (text, [0, 300, 500]), THRE, THRE)
    with pytest.raises(TypeError):
        KT.read_bins(t.M, None, reads, THRE, THRE)
    # and nothing above has changed what a good call returns
    check(KT.read_bins(t.M, t.P, reads, THRE, THRE), t.want(reads), "after the refusals")
