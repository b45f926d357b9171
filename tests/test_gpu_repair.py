"""GPU: the repair stage.  KmerTable.apply_edits (repair_apply_kernel alone) against plain Python slicing, aimed at the kernel's tile
seams, its misaligned loads and its edit chunks; KmerTable.repair / repair_device against the restatement of test_repair_host.py, fed by
Python dicts of canonical k-mer strings, with the round invariants asserted on the GPU's own reports.  Nothing expected here comes from
the code under test."""
import numpy as np
import pytest

from golden_util import case_names
from test_gpu_copies import is_wide
from test_indels_host import rand_bases
from test_repair_host import ANCHORS, FUZZ, apply_edits, check_invariants, fuzz_repair, golden_repair, pairs_repair, texts_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def KT(hip):
    from jasper_amd import KmerTable
    return KmerTable


@pytest.fixture(scope="module")
def T(KT):
    t = KT.repair_tile_bytes()
    assert t >= 1024 and t % 16 == 0
    return t


@pytest.fixture(scope="module")
def tab(KT):
    """apply_edits reads no count: any table does"""
    t = KT(21, min_slots=1 << 16)
    yield t
    t.close()


def applies(tab, seqs, edits):
    """apply_edits on [(seq, pos, rlen, y)] against slicing"""
    from jasper_amd.table import make_edits
    got = tab.apply_edits(seqs, make_edits(edits))
    want = apply_edits(seqs, edits)
    assert [len(g) for g in got] == [len(w) for w in want]
    assert got == want
    return got


def text(n, seed=1):
    return rand_bases(np.random.default_rng(seed), n)


# ---- the apply kernel against slicing ----------------------------------------------------------------------------------------------
def test_edits_at_the_tile_seams(tab, T):
    s = text(3 * T + 5)
    y64 = text(64, 2).decode()
    applies(tab, [s], [(0, T - 30, 0, y64)])              # 64 inserted bases whose output straddles byte T
    applies(tab, [s], [(0, T - 32, 64, "")])              # 64 deleted bytes across input byte T
    applies(tab, [s], [(0, T - 1, 1, "G")])               # ends at output byte T - 1
    applies(tab, [s], [(0, T, 0, "GATTACA")])             # starts at output byte T
    applies(tab, [s], [(0, T, 5, "")])
    applies(tab, [s], [(0, T - 1, 1, "G"), (0, T + 1, 1, "C"), (0, 2 * T - 64, 64, y64), (0, 2 * T + 1, 64, ""), (0, 3 * T + 4, 1, "TT")])
    applies(tab, [s], [(0, 0, 0, y64), (0, 3 * T + 5, 0, y64)])      # before the first byte and after the last
    applies(tab, [s], [(0, 0, 3 * T + 5, "")])            # everything goes
    applies(tab, [s], [(0, 0, 3 * T + 5, "ACG")])
    applies(tab, [s[:T]], [])                             # exactly one tile, one byte less, one more
    applies(tab, [s[:T - 1]], [(0, 7, 1, "A")])
    applies(tab, [s[:T + 1]], [(0, 7, 1, "A")])


def test_every_source_misalignment(tab, T):
    s = text(2 * T + 9, 3)
    for d in range(1, 16):
        applies(tab, [s], [(0, 5, 0, "ACGTACGTACGTACGT"[:d])])       # the tile after reads d bytes back ...
        applies(tab, [s], [(0, 5, d, "")])                           # ... or ahead
    # and all of them in one call: the deltas add up to 1, 3, 6, .. -- every residue of 16 but 0
    seqs = [text(T + 40 + i, 10 + i) for i in range(15)]
    applies(tab, seqs, [(i, 3 + i, 0, "ACGTACGTACGTACGT"[:i + 1]) for i in range(15)])


def test_many_short_sequences_in_one_tile(tab, T):
    rng = np.random.default_rng(4)
    seqs = [rand_bases(rng, int(n)) for n in rng.integers(0, 41, 300)]
    seqs[0] = seqs[7] = seqs[299] = b""
    assert sum(len(s) for s in seqs) < 2 * T and sum(1 for s in seqs if not s) >= 3
    edits = []
    for i, s in enumerate(seqs):
        if i % 3 == 0 and len(s) >= 12:
            edits += [(i, 0, 1, "T"), (i, 5, 2, ""), (i, len(s), 0, "GG")]      # a sequence's first byte, and an insertion at its end
        elif i % 3 == 1 and len(s) >= 1:
            edits.append((i, len(s) - 1, 1, ""))                                  # the last byte goes: the next sequence's edit may follow at once
        elif i % 7 == 2:
            edits.append((i, 0, 0, "ACGTT"))                                      # also into empty sequences
    assert len(edits) > 100 and any(not seqs[e[0]] for e in edits)
    applies(tab, seqs, edits)
    applies(tab, seqs, [])
    applies(tab, [], [])
    applies(tab, [b"", b""], [])
    applies(tab, [b""], [(0, 0, 0, "ACGT")])


def test_tiles_touched_by_many_edits(tab, T):
    s = text(2 * T + 100, 5)
    applies(tab, [s], [(0, p, 1, "ACGT"[(p >> 1) & 3]) for p in range(0, 2 * T + 100, 2)])      # T / 2 substitutions a tile
    # 64-byte deletions with 1-byte gaps: every OUTPUT byte has an edit of its own, a tile goes through its chunks of edits in a loop
    n = T + 300
    s = text(65 * n + 3, 6)
    applies(tab, [s], [(0, 65 * i + 1, 64, "") for i in range(n)])
    applies(tab, [s[:65 * (T // 65 + 1) + 3]], [(0, 65 * i + 1, 64, "") for i in range(T // 65 + 1)])      # the deletions that touch one INPUT tile
    # insertions of 64 with 1-byte gaps: 65 output bytes an edit
    s = text(3 * T // 65 + 50, 7)
    applies(tab, [s], [(0, 2 * i, 0, text(64, 100 + i).decode()) for i in range(len(s) // 2)])


def test_bytes_that_are_not_replaced_stay(tab, T):
    s = bytearray(text(T + 500, 8))
    s[100:160] = bytes(s[100:160]).lower()
    s[200:210] = b"NNNNNnnnnn"
    s[T - 8:T + 8] = b"acgtNnRyKm-*xXzZ"
    s = bytes(s)
    assert applies(tab, [s], [])[0] == s
    got = applies(tab, [s], [(0, 50, 1, "A"), (0, 130, 3, "GG"), (0, 205, 0, "T"), (0, T + 100, 2, "")])[0]
    assert got[:50] == s[:50] and b"NNNNNTnnnnn" in got and got[T - 8:T + 8] == s[T - 8:T + 8]      # (the three edits before add up to 0)
    assert bytes(got[130:132]) == b"GG"                   # y is written in upper case among lower-case neighbours


def random_edit_set(rng, lens):
    edits = []
    for si, n in enumerate(lens):
        pos = int(rng.integers(0, 40))
        while pos <= n:
            rlen = int(rng.integers(0, 70)) if rng.random() < 0.3 else int(rng.integers(0, 3))
            rlen = min(rlen, n - pos)
            ylen = int(rng.integers(0, 65)) if rng.random() < 0.3 else int(rng.integers(0, 3))
            if rlen + ylen:
                edits.append((si, pos, rlen, rand_bases(rng, ylen).decode()))
            pos += rlen + 1 + int(rng.integers(0, 200) if rng.random() < 0.8 else rng.integers(0, 3))
    return edits


def test_random_legal_edit_sets(tab, T):
    rng = np.random.default_rng(9)
    s = text(4 * T, 9)
    total = 0
    for it in range(50):
        seqs = [s] if it % 2 == 0 else [s[:T + 17], b"", s[T + 17:3 * T - 1], s[3 * T - 1:]]
        edits = random_edit_set(rng, [len(x) for x in seqs])
        total += len(edits)
        applies(tab, seqs, edits)
    assert total > 2000


def test_a_text_in_hbm_that_does_not_start_at_offset_zero(tab, T):
    import torch
    from jasper_amd.table import make_edits
    s = text(2 * T + 77, 11)
    d = torch.frombuffer(bytearray(b"xxxxx" + s + b"yyy"), dtype=torch.uint8).to("cuda:%d" % tab.device)
    offs = [5, 5 + T - 3, 5 + T - 3, 5 + len(s)]
    seqs = [s[:T - 3], b"", s[T - 3:]]
    edits = [(0, 10, 3, "A"), (0, T - 3, 0, "CCC"), (2, 0, 1, ""), (2, 50, 0, text(64, 12).decode())]
    got = tab.apply_edits_device(d, offs, make_edits(edits))
    torch.cuda.synchronize()
    assert got == apply_edits(seqs, edits)
    assert bytes(d.cpu().numpy().tobytes()) == b"xxxxx" + s + b"yyy"      # the input text is not written


def test_illegal_lists_are_errors_and_write_nothing(tab, T):
    from jasper_amd import _lib
    from jasper_amd.table import make_edits
    seqs = [text(50, 13), text(40, 14)]
    good = [(0, 10, 2, "AC"), (0, 20, 0, "G"), (1, 5, 3, "")]
    keep = [bytes(s) for s in seqs]

    def refused(arr, what):
        with pytest.raises(_lib.JasperHipError, match=what):
            tab.apply_edits(seqs, arr)
        assert seqs == keep

    refused(make_edits([good[1], good[0], good[2]]), "order")
    refused(make_edits([good[2], good[0]]), "order")
    refused(make_edits([(0, 10, 2, "AC"), (0, 12, 0, "G")]), "less than one byte apart")
    refused(make_edits([(1, 38, 3, "")]), "beyond its sequence")
    refused(make_edits([(0, 51, 0, "A")]), "beyond its sequence")
    refused(make_edits([(0, -1, 1, "A")]), "beyond its sequence")
    refused(make_edits([(2, 0, 1, "A")]), "no sequence")
    a = make_edits(good)
    a["len"][0] = 65
    refused(a, "more than 64")
    a = make_edits(good)
    a["bases"][0][0] |= 1 << 4
    refused(a, "bits above")
    a = make_edits(good)
    a["bases"][0][1] = 1
    refused(a, "bits above")
    assert tab.apply_edits(seqs, make_edits(good)) == apply_edits(seqs, good)      # and the table still works


# ---- the loop against the restatement ------------------------------------------------------------------------------------------------
def check_repair(rp, seqs, want, k, count, thre, what):
    assert rp.edit_tuples() == want["edits"], what
    assert rp.seqs == want["seqs"], what
    assert rp.rounds == want["rounds"], what
    for rep, w in ((rp.before, want["before"]), (rp.after, want["after"])):
        assert rep.counts == w[0] and rep.run_tuples() == w[1], what
    assert all(bytes(e["pad"]) == bytes(4) for e in rp.edits)
    assert 0 <= rp.apply_seconds <= rp.seconds
    # the invariants on the GPU's own reports
    check_invariants(texts_of(seqs, rp.edit_tuples()), rp.edit_tuples(), rp.rounds, k, count, thre)
    assert rp.rounds[0][4] == sum(c[2] for c in rp.before.counts) and rp.rounds[-1][5] == sum(c[2] for c in rp.after.counts)


@pytest.mark.parametrize("name", case_names())
def test_golden_cases(KT, name):
    c, seqs, count, want = golden_repair(name)
    assert [(rt[1], rt[2], rt[4], rt[5]) for rt in want["rounds"] if rt[1]] == ANCHORS[name]
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    rp = t.repair(seqs, c.thre)
    check_repair(rp, seqs, want, c.k, count, c.thre, name)
    assert rp.before == t.kmer_report(seqs, c.thre) and rp.after == t.kmer_report(rp.seqs, c.thre)
    assert rp == t.repair(seqs, c.thre, 4, 64, 3)         # determinism: two calls give equal results
    t.close()


def test_one_round_on_cluster_k25(KT):
    c, seqs, count, want = golden_repair("cluster_k25", 1)
    assert want["rounds"] == [(13, 12, 1, 0, 450, 68)]
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    rp = t.repair(seqs, c.thre, rounds=1)
    check_repair(rp, seqs, want, c.k, count, c.thre, "one round")
    assert len(rp.edits) == 12 and rp.after == t.kmer_report(rp.seqs, c.thre)      # `after` from one more report
    t.close()


def test_repair_device_gives_the_same(KT):
    import torch
    c, seqs, count, want = golden_repair("cluster_k25")
    t = KT(c.k, min_slots=1 << 16)
    t.count_text(c.reads_text())
    raw = b"".join(s.encode() for s in seqs)
    offs = [3]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(b"NNN" + raw + b"N"), dtype=torch.uint8).to("cuda:%d" % t.device)
    rp = t.repair_device(d, offs, c.thre)
    torch.cuda.synchronize()
    check_repair(rp, seqs, want, c.k, count, c.thre, "device")
    assert rp == t.repair(seqs, c.thre) and d.cpu().numpy().tobytes() == b"NNN" + raw + b"N"
    t.close()


@pytest.mark.parametrize("k", [21, 31, 64])
def test_planted_pairs(KT, k):
    truth, contig, pairs, far, count, want = pairs_repair(k)
    if k < 64:
        assert want["rounds"][0][:4] == (11, 10, 1, 0) and want["seqs"] == [truth]
    t = KT(k, min_slots=1 << 16)
    t.count_bases(b"N".join([truth] * 5))
    check_repair(t.repair([contig], 3), [contig], want, k, count, 3, k)
    t.close()


def test_a_wide_table_at_k41(KT):
    truth, contig, pairs, far, count, want = pairs_repair(41)
    assert want["seqs"] == [truth] and len(want["edits"]) >= 10
    t = KT(41, min_slots=1 << 16)
    t.count_bases(b"N".join([truth] * 5))
    assert is_wide(t)
    check_repair(t.repair([contig], 3), [contig], want, 41, count, 3, 41)
    t.close()


def test_tiny_fuzz(KT):
    seen = dict(two_rounds=0, conflicts=0, edits=0)
    tables = {}
    for k, seed, thre in FUZZ:
        reads, seqs, count, want = fuzz_repair(k, seed, thre)
        t = tables.setdefault(k, KT(k, min_slots=1 << 16))
        if thre == 1:                                     # (thre 2 follows with the same reads)
            t.clear()
            t.count_bases(b"N".join(reads))
        check_repair(t.repair(seqs, thre, 4, 8, 3), seqs, want, k, count, thre, (k, seed, thre))
        seen["two_rounds"] += sum(1 for rt in want["rounds"] if rt[1]) >= 2
        seen["conflicts"] += sum(rt[2] for rt in want["rounds"])
        seen["edits"] += len(want["edits"])
    for t in tables.values():
        t.close()
    assert seen["two_rounds"] >= 1 and seen["conflicts"] >= 1 and seen["edits"] > 100, seen


def test_bad_arguments_are_errors(KT):
    from jasper_amd import _lib
    t = KT(31, min_slots=1 << 16)
    t.count_bases(b"ACGT" * 100)
    seqs = ["ACGT" * 50]
    for s in (seqs, []):
        with pytest.raises(_lib.JasperHipError, match="thre"):
            t.repair(s, 0)
        for bad in (0, 9, -1):
            with pytest.raises(_lib.JasperHipError, match="rounds"):
                t.repair(s, 1, rounds=bad)
        with pytest.raises(_lib.JasperHipError, match="indel_max_len"):
            t.repair(s, 1, indel_max_len=17)
        with pytest.raises(_lib.JasperHipError, match="compound_max_len"):
            t.repair(s, 1, compound_max_len=65)
    rp = t.repair(seqs, 1)
    assert rp.seqs == [seqs[0].encode()] and len(rp.edits) == 0 and rp.rounds == [(0, 0, 0, 0, 0, 0)] and rp.before == rp.after
    assert t.repair([], 1).seqs == []
    t.close()
    t1 = KT(1, min_slots=1 << 16)
    with pytest.raises(_lib.JasperHipError, match="k must"):
        t1.repair(seqs, 1)
    t1.close()
