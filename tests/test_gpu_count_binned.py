"""GPU: the reads of chosen bins of a packed batch counted into tables (KmerTable.count_binned / count_binned_device /
count_binned_workspace, jasper_count_binned, csrc/bincount.hip).  Every sink's exported table is compared, as a dict, with a Counter of
canonical k-mer strings over the selected reads (tests/layout_util.py: kmer_counter); nothing expected here comes from the code under test.

What the gather kernel can get wrong is where reads begin and end in a stream it writes 16 aligned bytes at a time, so the reads here
have every length around a group (0, 1, 15, 16, 17, 63 .. 65, 255 .. 257), around k, and one of 70 000 bases; the selected reads begin on
every offset of a 16-byte group in the text and in the stream; and a piece of 256 bytes ends after every few reads."""
import collections
import os

import numpy as np
import pytest

import layout_util as lu

pytestmark = pytest.mark.gpu

KS = [21, 41]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LONG = 70000


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


class env:
    """an environment variable for the duration of a block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def rand_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


class Batch:
    """reads of the lengths above cut from a genome of 2500 bases (so k-mers repeat between reads and bins), some with lower case and
    N inside, the long read in the middle; codes that alternate 0, 1, 2 with a run of 40 reads of code 2 and one of 40 of code 0; and
    per bin the Counter of its reads' k-mers"""

    def __init__(self, k, seed):
        rng = np.random.default_rng(seed)
        self.k = k
        genome = rand_seq(rng, 2500)
        lens = [0, 1, k - 1, k, k + 1, 15, 16, 17, 63, 64, 65, 255, 256, 257]
        reads = []
        for i in range(25 * len(lens)):
            n = lens[i % len(lens)]
            p = int(rng.integers(0, len(genome) - n + 1))
            r = bytearray(genome[p:p + n])
            if n > k and i % 5 == 0:
                r[n // 2] = ord("N")
            if n > k and i % 7 == 0:
                r[:n // 3] = bytes(r[:n // 3]).lower()
            reads.append(bytes(r))
        reads.insert(len(reads) // 2, rand_seq(rng, LONG))
        codes = [i % 3 for i in range(len(reads))]
        codes[60:100] = [2] * 40
        codes[200:240] = [0] * 40
        self.reads, self.codes = reads, np.array(codes, dtype=np.uint8)
        self.by_bin = [lu.kmer_counter(b"\n".join(r for r, c in zip(reads, codes) if c == b), k) for b in range(3)]
        assert codes[0] == 0 and codes[-1] != 0 and len(reads[len(reads) // 2]) == LONG
        assert all(len(d) > 1000 for d in self.by_bin) and any(c > 3 for c in self.by_bin[1].values())

    def want(self, bins):
        d = collections.Counter()
        for b in bins:
            d.update(self.by_bin[b])
        return dict(d)

    def stats(self, bins):
        sel = [r for r, c in zip(self.reads, self.codes) if c in bins]
        return len(sel), sum(len(r) for r in sel), sum(self.want(bins).values())


@pytest.fixture(scope="module")
def batches():
    return {k: Batch(k, 900 + k) for k in KS}


def tables(KT, k, n):
    return [KT(k, min_slots=1 << 16) for _ in range(n)]


def close(*ts):
    for t in ts:
        t.close()


def check_sinks(ts, sinks_bins, B, stats):
    for t, bins, st in zip(ts, sinks_bins, stats):
        got, want = lu.table_dict(t), B.want(bins)
        assert got == want, (bins, lu._diff(got, want))
        assert (st["reads"], st["bases"], st["occurrences"]) == B.stats(bins), bins
        assert st["gather_seconds"] > 0 and st["count_seconds"] > 0


@pytest.mark.parametrize("k", KS)
def test_three_sinks_in_one_call(KT, batches, k):
    """{0}, {1} and {0,1,2} in one call: as dicts, and all == the sum of the three bins ({2} from a call of its own: its first read is
    not selected, its last may be)"""
    B = batches[k]
    ts = tables(KT, k, 4)
    bins = [(0,), (1,), (0, 1, 2)]
    st = KT.count_binned(B.reads, B.codes, list(zip(ts[:3], bins)))
    check_sinks(ts[:3], bins, B, st)
    st2 = KT.count_binned(B.reads, B.codes, [(ts[3], (2,))])
    check_sinks(ts[3:], [(2,)], B, st2)
    total = collections.Counter()
    for t in (ts[0], ts[1], ts[3]):
        total.update(lu.table_dict(t))
    assert dict(total) == lu.table_dict(ts[2])
    assert st[2]["reads"] == len(B.reads) == st[0]["reads"] + st[1]["reads"] + st2[0]["reads"]
    # a second call adds to what a table holds
    KT.count_binned(B.reads, B.codes, [(ts[0], 0b001)])
    assert lu.table_dict(ts[0]) == {km: 2 * c for km, c in B.want((0,)).items()}
    close(*ts)


@pytest.mark.parametrize("k", KS)
def test_pieces_of_256_bytes(KT, batches, k):
    """a piece ends after every few reads (a read of 255 .. 257 bases with its separator fills or overflows one) and the long read is a
    piece of its own: no k-mer is lost or made at a seam"""
    B = batches[k]
    ts = tables(KT, k, 3)
    bins = [(0, 2), (1,), (1, 2)]
    with env(JASPER_BINCOUNT_PIECE="256"):
        st = KT.count_binned(B.reads, B.codes, list(zip(ts, bins)))
    check_sinks(ts, bins, B, st)
    for bad in ("0", "x", "", str((1 << 36) + 1)):
        with env(JASPER_BINCOUNT_PIECE=bad):
            with pytest.raises(Exception, match="JASPER_BINCOUNT_PIECE must be a number of bytes"):
                KT.count_binned(B.reads, B.codes, [(ts[0], (0,))])
    close(*ts)


@pytest.mark.parametrize("k", KS)
def test_all_none_and_no_reads(KT, batches, k):
    B = batches[k]
    t, u = tables(KT, k, 2)
    one = np.zeros(len(B.reads), dtype=np.uint8)
    st = KT.count_binned(B.reads, one, [(t, (0,)), (u, (1, 2))])          # all selected; none selected
    assert lu.table_dict(t) == B.want((0, 1, 2)) and st[0]["reads"] == len(B.reads)
    assert lu.table_dict(u) == {} and u.info()["distinct"] == 0 and (st[1]["reads"], st[1]["bases"], st[1]["occurrences"]) == (0, 0, 0)
    st = KT.count_binned([], [], [(u, (0, 1, 2))])
    assert lu.table_dict(u) == {} and st[0]["reads"] == 0
    st = KT.count_binned([b"", b"A", b"ACGT" * 5, b""], [0, 0, 0, 0], [(u, (0,))])      # only reads shorter than k
    assert lu.table_dict(u) == {} and (st[0]["reads"], st[0]["bases"], st[0]["occurrences"]) == (4, 21, 0)
    close(t, u)


@pytest.mark.parametrize("k", KS)
def test_junction_of_two_selected_reads(KT, k):
    """x is planted once inside a read; at every cut c the reads (.. x[:c]) and (x[c:] ..) follow each other in the stream, both
    selected, with an unselected read between them in the text: the junction must not count as x"""
    rng = np.random.default_rng(300 + k)
    x, pre, post = rand_seq(rng, k), rand_seq(rng, 23), rand_seq(rng, 29)
    reads, codes = [pre + x + post], [1]
    for c in range(1, k):
        reads += [pre + x[:c], rand_seq(rng, 40), x[c:] + post]
        codes += [1, 0, 1]
    t, = tables(KT, k, 1)
    KT.count_binned(reads, codes, [(t, (1,))])
    want = dict(lu.kmer_counter(b"\n".join(r for r, c in zip(reads, codes) if c == 1), k))
    got = lu.table_dict(t)
    canon = lu.canon(x.decode())
    assert want[canon] == 1 and got == want, lu._diff(got, want)
    close(t)


@pytest.mark.parametrize("k", KS)
def test_entry_points_and_alignment(KT, batches, k):
    """the text 1, 3 and 15 bytes off a 16-byte boundary through the host pointer and through the device pointer; the workspace entry
    after read_bins_text on FASTQ text of the same reads; all equal the host entry's tables"""
    import torch
    B = batches[k]
    bins = [(0,), (1, 2)]
    want = [B.want(b) for b in bins]
    text = b"".join(B.reads)
    offs = np.zeros(len(B.reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in B.reads], out=offs[1:])
    for shift in (1, 3, 15):
        buf = np.frombuffer(bytearray(b"T" * (len(text) + 64)), dtype=np.uint8)
        start = (shift - buf.ctypes.data) % 16                            # the first read's first byte lies `shift` bytes behind a boundary
        buf[start:start + len(text)] = np.frombuffer(text, dtype=np.uint8)
        assert (buf.ctypes.data + start) % 16 == shift
        ts = tables(KT, k, 2)
        KT.count_binned((buf, offs + start), B.codes, list(zip(ts, bins)))
        assert [lu.table_dict(t) for t in ts] == want, shift
        close(*ts)
        d = torch.frombuffer(bytearray(b"\x00" * 16 + b"T" * shift + text + b"ACGT" * 8), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        ts = tables(KT, k, 2)
        st = KT.count_binned_device(d.data_ptr() + 16, offs + shift, B.codes, list(zip(ts, bins)))
        assert [lu.table_dict(t) for t in ts] == want, shift
        assert st[0]["reads"] == B.stats(bins[0])[0]
        close(*ts)
    # the workspace entry: FASTQ text of the same reads, parsed and packed on the GPU by a binning call on two tables of its own
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(B.reads))
    mat, pat = tables(KT, k, 2)
    mat.count_bases(b"ACGT" * 20)
    pat.count_bases(b"AACC" * 20)
    r = KT.read_bins_text(mat, pat, fq, True, "fastq", 1, 1)
    assert r.n_records == len(B.reads) and not r.malformed and r.lens.tolist() == [len(x) for x in B.reads]
    with env(JASPER_BINCOUNT_PIECE="4096"):
        ts = tables(KT, k, 2)
        st = KT.count_binned_workspace(mat, pat, r.n_records, B.codes, list(zip(ts, bins)))
    assert [lu.table_dict(t) for t in ts] == want
    assert [(s["reads"], s["bases"], s["occurrences"]) for s in st] == [B.stats(b) for b in bins]
    # refusals of the workspace entry
    with pytest.raises(Exception, match="n_records is not what the read-text call returned"):
        KT.count_binned_workspace(mat, pat, r.n_records - 1, B.codes[:-1], [(ts[0], (0,))])
    with pytest.raises(Exception, match="one of the binning's own tables"):
        KT.count_binned_workspace(mat, pat, r.n_records, B.codes, [(mat, (0,))])
    with pytest.raises(Exception, match="one of the binning's own tables"):
        KT.count_binned_workspace(mat, pat, r.n_records, B.codes, [(ts[0], (0,)), (pat, (1,))])
    assert [lu.table_dict(t) for t in ts] == want                          # nothing was touched
    KT.read_bins(mat, pat, [b"ACGT" * 30], 1, 1)                          # any binning call since: nothing is left to count
    with pytest.raises(Exception, match="no read-text call has left anything to count"):
        KT.count_binned_workspace(mat, pat, r.n_records, B.codes, [(ts[0], (0,))])
    close(mat, pat, *ts)


def test_refusals(KT):
    k = 21
    reads = [b"ACGTTGCA" * 8, b"TTGACCA" * 9, b""]
    t, u = tables(KT, k, 2)
    other_k = KT(k + 2, min_slots=1 << 16)
    with pytest.raises(Exception, match="different k"):
        KT.count_binned(reads, [0, 1, 2], [(t, (0,)), (other_k, (1,))])
    with pytest.raises(Exception, match="sinks 0 and 1 are the same table"):
        KT.count_binned(reads, [0, 1, 2], [(t, (0,)), (t, (1,))])
    with pytest.raises(Exception, match="a bin code is not 0, 1 or 2"):
        KT.count_binned(reads, [0, 3, 2], [(t, (0,))])
    for mask in (0, 8, 255):
        with pytest.raises(Exception, match="must be 1 to 7"):
            KT.count_binned(reads, [0, 1, 2], [(t, mask)])
    with pytest.raises(Exception, match="must be 1 to 7"):
        KT.count_binned(reads, [0, 1, 2], [(t, (0, 3))])
    with pytest.raises(Exception, match="offsets must not decrease"):
        KT.count_binned((b"ACGT" * 100, [0, 300, 200]), [0, 1], [(t, (0,))])
    with pytest.raises(Exception, match="1 to 3 sinks"):
        KT.count_binned(reads, [0, 1, 2], [])
    with pytest.raises(Exception, match="1 to 3 sinks"):
        KT.count_binned(reads, [0, 1, 2], [(t, 1), (u, 2), (other_k, 4), (t, 7)])
    with pytest.raises(Exception, match="null text"):
        KT.count_binned_device(0, [0, 300], [0], [(t, (0,))])
    with pytest.raises(ValueError, match="one bin code per read"):
        KT.count_binned(reads, [0, 1], [(t, (0,))])
    with pytest.raises(TypeError, match="sink table must be an open KmerTable"):
        KT.count_binned(reads, [0, 1, 2], [(None, (0,))])
    assert lu.table_dict(t) == {} and lu.table_dict(u) == {}             # nothing was counted by a refused call
    close(t, u, other_k)


def test_an_attached_sink_is_refused(KT):
    from test_gpu_shard import make_shards
    k = 21
    src = KT(k, min_slots=1 << 16)
    src.count_bases(bytes(rand_seq(np.random.default_rng(5), 3000)))
    shards, _ = make_shards(KT, src, 2, src.info()["slots"])
    for o, sh in enumerate(shards):
        sh.attach_tables(shards, o)
    with pytest.raises(Exception, match="must be a whole table, not an attached owner-sharded one"):
        KT.count_binned([b"ACGT" * 10], [0], [(shards[0], (0,))])
    close(src, *shards)
