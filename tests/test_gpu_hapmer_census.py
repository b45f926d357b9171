"""GPU: the hap-mer census (KmerTable.hapmer_census / hapmer_census_parents, jasper_hapmer_census) against a restatement of its semantics
fed by Python dicts of canonical k-mer strings.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): H_mat = the distinct keys x of the mother's table M with M[x] >= thre_mat, P[x] == 0 and (no child
table or R[x] >= thre_child), counts clamped to 2^32-1; H_pat the same with the parents swapped.  For each: hapmers = |H|, found = the
keys of H with A[x] >= 1, occurrences = the sum over H of A[x]; found and occurrences are 0 without an assembly table.

The restatement is this file's own (canon, windows, kmer_dict, census, scan_totals); from test_gpu_hapmers.py come only the workload --
the trio's three texts and the tables counted from them -- not a dict and not a classifier."""
import collections

import pytest

from test_gpu_hapmers import DEPTH, THRE, TILE, Trio, depth, rand_seq, table

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def canon(km):
    return min(km, km.translate(_RC)[::-1])


def windows(seq, k):
    """the canonical k-mers of the valid windows of one sequence, in order (case folded; a window with any other byte is skipped)"""
    b = bytes(seq).upper()
    for i in range(len(b) - k + 1):
        w = b[i:i + k]
        if not w.strip(b"ACGT"):
            yield canon(w)


def kmer_dict(texts, k, times=1):
    d = collections.Counter()
    for t in texts:
        for key in windows(t, k):
            d[key] += times
    return d


def hapmer_sets(md, pd, cd, tm, tp, tc):
    return [{x for x, c in own.items() if min(c, U32) >= thre and other.get(x, 0) == 0 and (cd is None or min(cd.get(x, 0), U32) >= tc)}
            for own, other, thre in ((md, pd, tm), (pd, md, tp))]


def scan_totals(seqs, k, md, pd, cd, tm, tp, tc):
    """(mat windows, pat windows) of the scan over the sequences: the windows whose k-mer is a hap-mer of that parent"""
    hm, hp = hapmer_sets(md, pd, cd, tm, tp, tc)
    keys = [key for s in seqs for key in windows(s, k)]
    return sum(key in hm for key in keys), sum(key in hp for key in keys)


def trio_dicts(t):
    """the three dicts of a Trio's texts: the parents at depth DEPTH, the child both haplotypes twice"""
    return kmer_dict([t.mat_hap], t.k, DEPTH), kmer_dict([t.pat_hap], t.k, DEPTH), kmer_dict([t.mat_hap, t.pat_hap], t.k, 2)


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


def census(md, pd, cd, ad, tm, tp, tc):
    """((hapmers, found, occurrences) of mat, ... of pat)"""
    out = []
    for own, other, thre in ((md, pd, tm), (pd, md, tp)):
        H = [x for x, c in own.items() if min(c, U32) >= thre and other.get(x, 0) == 0 and (cd is None or min(cd.get(x, 0), U32) >= tc)]
        if ad is None:
            out.append((len(H), 0, 0))
        else:
            out.append((len(H), sum(1 for x in H if ad.get(x, 0) >= 1), sum(min(ad.get(x, 0), U32) for x in H)))
    return tuple(out)


@pytest.mark.parametrize("k", [25, 41])
def test_census_of_a_trio(KT, k):
    t = Trio(KT, 700 + k, k, 3 * TILE + 100 if k == 25 else TILE + 50)
    seqs = [t.contig, t.pat_hap[-3000:]]            # (the contig's second half is the paternal haplotype: its hap-mers there occur twice)
    A = table(KT, k, b"N".join(seqs))
    ad = kmer_dict(seqs, k)
    md, pd, cd = trio_dicts(t)
    for child in (True, False):
        for asm in (True, False):
            want = census(md, pd, cd if child else None, ad if asm else None, THRE, THRE, THRE)
            got = t.R.hapmer_census(t.M, t.P, A if asm else None, THRE, THRE, THRE, child=child)
            print(k, child, asm, want, (got.mat, got.pat), got.seconds)
            assert (got.mat, got.pat) == want, (k, child, asm)
            assert got.seconds > 0
    want = census(md, pd, None, ad, THRE, THRE, 1)
    assert want[0][0] > 500 and want[1][0] > 500 and 0 < want[0][1] < want[0][0] and 0 < want[1][1] < want[1][0], "vacuous case"
    assert want[1][2] > want[1][1], "no paternal hap-mer occurs twice in the assembly"
    got = KT.hapmer_census_parents(t.M, t.P, A, THRE, THRE)
    assert (got.mat, got.pat) == want
    # a threshold above the depth: no hap-mer at all; and thresholds of 1
    got = t.R.hapmer_census(t.M, t.P, A, DEPTH + 1, THRE, THRE)
    assert (got.mat, got.pat) == census(md, pd, cd, ad, DEPTH + 1, THRE, THRE) and got.mat == (0, 0, 0)
    got = t.R.hapmer_census(t.M, t.P, A, 1, 1, 3)
    assert (got.mat, got.pat) == census(md, pd, cd, ad, 1, 1, 3) and got.mat == (0, 0, 0), "the child holds every k-mer twice"
    # the free cross-check between the two kernels: A counted from exactly the scanned contigs
    for child in (True, False):
        scan = t.R.hapmer_scan(t.M, t.P, seqs, THRE, THRE, THRE, child=child)
        cen = t.R.hapmer_census(t.M, t.P, A, THRE, THRE, THRE, child=child)
        assert cen.mat[2] == sum(c[2] for c in scan.counts) > 0 and cen.pat[2] == sum(c[3] for c in scan.counts) > 0
        assert (cen.mat[2], cen.pat[2]) == scan_totals(seqs, k, md, pd, cd if child else None, THRE, THRE, THRE)
    A.close()
    t.close()


def test_a_hapmer_twice_in_the_assembly(KT):
    """a maternal k-mer present twice in the assembly counts once in `found` and twice in `occurrences`"""
    import numpy as np
    k = 21
    rng = np.random.default_rng(5)
    mh, ph = bytes(rand_seq(rng, 300)), bytes(rand_seq(rng, 300))
    km = mh[40:40 + k]
    asm = mh[100:160] + b"N" + km + b"N" + km + b"N" + ph[:50]
    md, pd, ad = kmer_dict([mh], k, DEPTH), kmer_dict([ph], k, DEPTH), kmer_dict([asm], k)
    assert not set(md) & set(pd) and len(md) == len(pd) == 300 - k + 1 and ad[min(km, km.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])] == 2
    M, P, A = table(KT, k, depth(mh, DEPTH)), table(KT, k, depth(ph, DEPTH)), table(KT, k, asm)
    want = census(md, pd, None, ad, THRE, THRE, 1)
    assert want == ((300 - k + 1, 60 - k + 1 + 1, 60 - k + 1 + 2), (300 - k + 1, 50 - k + 1, 50 - k + 1))
    got = KT.hapmer_census_parents(M, P, A, THRE, THRE)
    assert (got.mat, got.pat) == want
    again = KT.hapmer_census_parents(M, P, A, THRE, THRE)
    assert again == got
    with pytest.raises(Exception, match="maternal table and the assembly table are the same table"):
        KT.hapmer_census_parents(M, P, M, THRE, THRE)
    with pytest.raises(Exception, match="paternal threshold must be at least 1"):
        KT.hapmer_census_parents(M, P, A, THRE, 0)
    other = table(KT, k + 2, asm)
    with pytest.raises(Exception, match="different k"):
        KT.hapmer_census_parents(M, P, other, THRE, THRE)
    other.close()
    for t in (M, P, A):
        t.close()


def test_an_attached_assembly_or_parent_is_refused_and_an_attached_child_is_swept(KT):
    """A, M and P must be whole tables; the child's may be an attached owner-sharded one, and the census through it is the whole table's"""
    from test_gpu_shard import make_shards
    k = 25
    t = Trio(KT, 4100, k, TILE // 2)
    md, pd, cd = trio_dicts(t)
    A = table(KT, k, t.contig)
    ad = kmer_dict([t.contig], k)
    shards, _ = make_shards(KT, t.R, 2, t.R.info()["slots"])
    for o, s in enumerate(shards):
        s.attach_tables(shards, o)
    want = census(md, pd, cd, ad, THRE, THRE, THRE)
    assert want[0][1] > 0 and want[1][1] > 0
    for s in shards:
        got = s.hapmer_census(t.M, t.P, A, THRE, THRE, THRE)
        assert (got.mat, got.pat) == want
    with pytest.raises(Exception, match="assembly table must be a whole table"):
        t.R.hapmer_census(t.M, t.P, shards[0], THRE, THRE, THRE)
    with pytest.raises(Exception, match="maternal table must be a whole table"):
        t.R.hapmer_census(shards[1], t.P, A, THRE, THRE, THRE)
    with pytest.raises(Exception, match="paternal table must be a whole table"):
        KT.hapmer_census_parents(t.M, shards[0], A, THRE, THRE)
    got = t.R.hapmer_census(t.M, t.P, A, THRE, THRE, THRE)
    assert (got.mat, got.pat) == want
    for s in shards + [A]:
        s.close()
    t.close()
