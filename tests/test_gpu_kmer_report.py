"""GPU: the dense k-mer report (KmerTable.kmer_report / kmer_report_device) against a restatement of its semantics that is
fed by an independent count source: the dict of a golden case's dump.txt.gz (printed by the real `jellyfish dump -c`) or
oracle.OracleDB.query.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h): window i of a sequence of n bytes exists for 0 <= i <= n-k; it is valid iff all k bytes are
ACGTacgt; its count is the canonical k-mer's, clamped to 2^32-1; unreliable = valid and count < thre; absent = valid and
count == 0; a run is a maximal range of consecutive unreliable windows: (seq, start, n_kmers, n_absent, min_count)."""
import numpy as np
import pytest

from golden_util import Case, case_names

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def window_counts(seq, k, count):
    """per window: None (not valid) or the clamped count; count(bytes of k upper-case bases) -> int"""
    b = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    n = len(b)
    pre = [0] * (n + 1)
    for i, ch in enumerate(b):
        pre[i + 1] = pre[i] + (0 if ch in b"ACGTacgt" else 1)
    up = b.upper()
    return [min(count(up[i:i + k]), U32) if pre[i + k] == pre[i] else None for i in range(max(0, n - k + 1))]


def restate(per_seq_counts, thre):
    """(counts, runs) of the semantics above from the per-window counts of every sequence"""
    counts, runs = [], []
    for si, wc in enumerate(per_seq_counts):
        valid = unrel = absent = 0
        cur = None
        for i, c in enumerate(wc):
            if c is not None:
                valid += 1
                absent += c == 0
            if c is not None and c < thre:
                unrel += 1
                if cur is None:
                    cur = [si, i, 0, 0, c]
                cur[2] += 1
                cur[3] += c == 0
                cur[4] = min(cur[4], c)
            elif cur is not None:
                runs.append(tuple(cur))
                cur = None
        if cur is not None:
            runs.append(tuple(cur))
        counts.append((len(wc), valid, unrel, absent))
    return counts, runs


def dump_counter(d):
    def count(km):
        rc = km.translate(_COMP)[::-1]
        return d.get(min(km, rc).decode(), 0)
    return count


def check(rep, want_counts, want_runs, what):
    assert rep.counts == want_counts, what
    got = rep.run_tuples()
    assert len(got) == len(want_runs), (what, len(got), len(want_runs))
    assert got == want_runs, what


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


# (windows, valid, unreliable, absent, runs) computed on the CPU from the cases' dumps
ANCHORS = {"cluster_k25": (5976, 5976, 450, 396, 14), "edges_k19": (3013, 2904, 168, 160, 10), "gaps_k37_p4": (5962, 5962, 1779, 1678, 35),
           "simple_k63": (3937, 3937, 575, 566, 11)}


def test_anchored_cases_exist():
    assert set(ANCHORS) <= set(case_names()) and len(case_names()) == 17


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c = Case(name)
    _, seqs = c.batch()
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    count = dump_counter(c.dump())
    want_counts, want_runs = restate([window_counts(s, c.k, count) for s in seqs], c.thre)
    rep = t.kmer_report(seqs, c.thre)
    t.close()
    check(rep, want_counts, want_runs, name)
    assert len(want_runs) >= 5, "vacuous case"
    if name in ANCHORS:
        tot = tuple(sum(x[i] for x in want_counts) for i in range(4)) + (len(want_runs),)
        assert tot == ANCHORS[name]
        assert tuple(sum(x[i] for x in rep.counts) for i in range(4)) + (len(rep.runs),) == ANCHORS[name]
    assert rep.seconds > 0


class DictDB:
    """canonical k-mer -> count in a Python dict: the count source where oracle.OracleDB has none (it takes k <= 63, the table
    k <= 64); the same two calls, as independent of the code under test as the oracle is"""

    def __init__(self, k):
        self.k, self.d = k, {}

    def count_bases(self, b):
        import re
        k, d = self.k, self.d
        for m in re.finditer(rb"[ACGT]{%d,}" % k, b.upper()):
            s = m.group()
            for i in range(len(s) - k + 1):
                km = s[i:i + k]
                rc = km.translate(_COMP)[::-1]
                key = km if km < rc else rc
                d[key] = d.get(key, 0) + 1

    def query(self, km):
        rc = km.translate(_COMP)[::-1]
        return self.d.get(km if km < rc else rc, 0)

    def histo(self):
        h = [0] * 10002
        for c in self.d.values():
            h[min(c, 10001)] += 1
        return h


def count_source(k):
    from oracle import oracle as O
    try:
        return O.OracleDB(k)
    except ValueError:
        assert k == 64
        return DictDB(k)


def derived_threshold(odb):
    from oracle import oracle as O
    h = odb.histo()
    try:
        thr = O.threshold([(m, h[m]) for m in range(1, 10002) if h[m]])
    except SystemExit:
        thr = None
    return thr if thr else 3


def fuzz_sequences(rng, k, genome, tile, count):
    """what the issue lists: N / n / lower case / other bytes, lengths < k, == k, empty, one tile +- 1, a run longer than a tile, a
    run that starts on a tile's last window, many short sequences"""
    from jasper_amd import synth
    ACGT = synth.ACGT
    asm = synth.make_assembly(rng, genome, err=2e-3, n_every=9000, n_len=40).copy()
    n = len(asm)
    a = int(rng.integers(0, n - 3000))
    asm[a:a + 2000] = np.frombuffer(asm[a:a + 2000].tobytes().lower(), dtype=np.uint8)      # lower case (and 'n' where an N stretch falls)
    for p, ch in zip(rng.integers(0, n, 12).tolist(), b"nRY-*.\n\0\xffxU "):
        asm[p] = ch
    seqs = [asm.tobytes()]
    g = genome.tobytes()
    seqs += [b"", g[100:100 + k - 1], g[200:200 + k], g[300:300 + k].lower()]
    if k > 1:
        seqs.append(g[:k - 1] + b"N" + g[k:2 * k - 1])                                        # no valid window at all
    for w in (tile - 1, tile, tile + 1):                                                       # exactly one tile of windows +- 1
        seqs.append(g[1000:1000 + w + k - 1])
    junk = ACGT[rng.integers(0, 4, int(2.5 * tile))].tobytes()                                 # not in the reads (k >= 17): a run across three tiles
    seqs.append(g[5000:5300] + junk + g[6000:6300])
    # window tile-1 is the first to hold a base that is not the genome's; the cut is put where the reads cover window tile-2, so that it ends no run
    g0 = next(p for p in range(7000, 8000) if count(g[p + tile - 2:p + tile - 2 + k]) > 0)
    cut = g0 + tile - 1 + k - 1
    other = b"C" if g[cut:cut + 1] != b"C" else b"G"                                          # (not the base the genome goes on with)
    seqs.append(g[g0:cut] + other + junk[:700])
    seqs.append(g[9000:9000 + 2 * tile - 1 + k - 1] + junk[:3] + g[20000:20000 + 3 * tile])    # the same at the second seam, short
    for _ in range(300):                                                                       # many short sequences
        p = int(rng.integers(0, n - 300))
        seqs.append(asm[p:p + int(rng.integers(0, 260))].tobytes())
    return seqs


def valid_stretches(seq, k):
    b = bytes(seq)
    n, run = 0, 0
    for ch in b:
        run = run + 1 if ch in b"ACGTacgt" else 0
        n += run == k
    return n


@pytest.mark.parametrize("k", [1, 17, 31, 32, 33, 37, 45, 63, 64])
def test_fuzz_against_oracle(KT, k):
    from jasper_amd import synth
    from oracle import oracle as O
    tile = KT.report_tile_windows()
    assert tile == 4096, "documented in include/jasper_hip.h"
    rng = np.random.default_rng(4200 + k)
    genome = synth.make_genome(rng, 60_000)
    reads = synth.make_reads_stream(rng, genome, 60, 150, 0.003).tobytes()
    odb = count_source(k)
    odb.count_bases(reads)
    seqs = fuzz_sequences(rng, k, genome, tile, odb.query)
    assert sum(len(s) for s in seqs) <= 300_000
    t = KT(k, min_slots=1 << 16)
    t.count_bases(reads)
    wcs = [window_counts(s, k, odb.query) for s in seqs]
    thr = derived_threshold(odb)
    seam = False
    for thre in (0, 1, thr, U32):
        want_counts, want_runs = restate(wcs, thre)
        rep = t.kmer_report(seqs, thre)
        check(rep, want_counts, want_runs, (k, thre))
        if thre == 0:
            assert len(rep.runs) == 0 and all(c[2] == 0 for c in rep.counts)
        if thre == 1:
            assert all(c[2] == c[3] for c in rep.counts)
        if thre == U32:
            assert len(rep.runs) == sum(valid_stretches(s, k) for s in seqs)
            assert max(int(r["n_kmers"]) for r in rep.runs) > 2 * tile                       # a run longer than a tile
        seam |= any(r[1] == tile - 1 and r[2] > 1 for r in want_runs)
    if k >= 17:
        assert seam, "no run starts on a tile's last window"
    # host text and device text give the same object
    import torch
    flat = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.kmer_report_device(d, offs, thr) == t.kmer_report(seqs, thr)
    t.close()


def test_more_runs_than_the_first_buffer_holds(KT):
    """every other window unreliable: the table holds the k-mers at the even positions of a random sequence only.  150 000 runs
    of one window each are more than the scan's first list of partial runs has room for (windows / 64 + 65 536)"""
    from oracle import oracle as O
    k = 21
    rng = np.random.default_rng(77)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300_000)].tobytes()
    reads = b"N".join(s[i:i + k] for i in range(0, len(s) - k + 1, 2))
    odb = O.OracleDB(k)
    odb.count_bases(reads)
    t = KT(k, min_slots=1 << 16)
    t.count_bases(reads)
    want_counts, want_runs = restate([window_counts(s, k, odb.query)], 1)
    assert len(want_runs) > 300_000 // 64 + 65_536
    rep = t.kmer_report([s], 1)
    check(rep, want_counts, want_runs, "alternating")
    assert rep.retried
    # every window unreliable: one run
    rep = t.kmer_report([s], U32)
    assert rep.run_tuples() == [(0, 0, len(s) - k + 1, want_counts[0][3], 0)]
    t.close()


def test_report_through_owner_shards_equals_whole_table(KT):
    from test_gpu_shard import make_shards, workload
    k = 37
    genome, reads, asm = workload(321, 200_000, k)
    full = KT(k, min_slots=1 << 21)
    full.count_bases(reads)
    shards, _ = make_shards(KT, full, 2, 1 << 21)
    for o, t in enumerate(shards):
        t.attach_tables(shards, o)
    seqs = [asm, asm[1000:90_000].lower(), asm[:36], ""]
    for thre in (1, 4, U32):
        want = full.kmer_report(seqs, thre)
        assert len(want.runs) >= 3
        assert shards[0].kmer_report(seqs, thre) == want
        assert shards[1].kmer_report(seqs, thre) == want
    for t in shards + [full]:
        t.close()


def test_ten_calls_give_identical_results(KT):
    from jasper_amd import synth
    k = 31
    rng = np.random.default_rng(9)
    genome = synth.make_genome(rng, 150_000)
    reads = synth.make_reads_stream(rng, genome, 15, 150, 0.004).tobytes()
    asm = synth.make_assembly(rng, genome, err=3e-3, n_every=40_000, n_len=30).tobytes()
    seqs = [asm[:100_000], asm[100_000:], asm[5:77], asm[50_000:70_000]]
    t = KT(k, min_slots=1 << 16)
    t.count_bases(reads)
    first = t.kmer_report(seqs, 3)
    assert len(first.runs) > 100
    for _ in range(9):
        assert t.kmer_report(seqs, 3) == first
    t.close()
