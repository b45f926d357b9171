"""CPU: the repair stage.  The restatement of its semantics that the GPU tests compare against (test_gpu_repair.py,
test_gpu_cli_repair.py), composed of the four scans' restatements and plain slicing; its selection checked against a plain form; the
three invariants of a round asserted on every input; anchors on the committed dumps of the golden cases; the host side
(jasper_amd/repair.py: the FASTA, the two TSVs, the log text; the flag errors of the driver) on hand-made edits; and the stand-alone
sanitizer build of the C++ selection (tools/repair_host_check.cpp).  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h, jasper_repair): an edit (seq, pos, rlen, y) replaces s[pos .. pos+rlen) by y; q = pos + rlen.  Only
records of kind error become edits: sub (p, alt) -> (p, 1, alt); ins(p, x, L) -> (p, 0, x^L); del(p, L) -> (p, L, ""); mixed ins(p, y)
-> (p, 0, y); compound (a, R, y) -> (a, R, y).  One round: indel scan with its mixed half (it carries the variant scan) and compound
scan on the current text; duplicates (seq, pos, rlen, y) dropped; edits that share (seq, pos, rlen, |y|, alt_min) and differ in y are
ambiguous and set aside; the rest in the order (rlen + |y|, -alt_min, seq, pos, rlen, y), each accepted unless it conflicts with an
accepted one -- a, b of one sequence with (pos_a, q_a) <= (pos_b, q_b) conflict iff pos_b - q_a < k - 1.  The accepted edits are applied;
a round that accepts nothing ends the loop; at most N rounds."""
import functools
import os
import subprocess
import sys

import pytest

from golden_util import Case, case_names
from test_compound_host import planted_pairs, restate_compound, tiny_fuzz
from test_gpu_copies import as_bytes, dict_counter, kmer_dict
from test_gpu_kmer_report import restate as restate_runs
from test_gpu_kmer_report import window_counts
from test_gpu_variants import restate as restate_variants
from test_indels_host import ERROR
from test_indels_host import restate as restate_indels
from test_indels_mixed_host import restate_mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("sub", "ins", "del", "mixed", "compound")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def normalise(variants, indels, mixed, compound):
    """the four record lists (tuples as the restatements give them) -> edits (seq, pos, rlen, y, alt_min, ref_min, source), error
    records only, in source order"""
    out = []
    for seq, pos, _ref, alt, rmin, amin, kind in variants:
        if kind == ERROR:
            out.append((seq, pos, 1, alt, amin, rmin, "sub"))
    for seq, pos, typ, ln, base, rmin, amin, kind in indels:
        if kind == ERROR:
            out.append((seq, pos, 0, base * ln, amin, rmin, "ins") if typ == "ins" else (seq, pos, ln, "", amin, rmin, "del"))
    for seq, pos, _ln, y, rmin, amin, kind in mixed:
        if kind == ERROR:
            out.append((seq, pos, 0, y, amin, rmin, "mixed"))
    for seq, pos, rlen, _ln, y, rmin, amin in compound:
        out.append((seq, pos, rlen, y, amin, rmin, "compound"))
    return out


def conflicts(a, b, k):
    """two edits of one sequence, whatever order they come in"""
    if a[0] != b[0]:
        return False
    x, y = sorted([a, b], key=lambda e: (e[1], e[1] + e[2]))
    return y[1] - (x[1] + x[2]) < k - 1


def select(edits, k):
    """(accepted in (seq, pos) order, records, conflicts, ambiguous) of one round.  Shortcut: the accepted edits of a sequence are kept
    sorted, and only the neighbours of a new edit in (pos, q) order are looked at"""
    import bisect
    uniq, seen = [], set()
    for e in edits:
        if e[:4] not in seen:
            seen.add(e[:4])
            uniq.append(e)
    groups = {}
    for e in uniq:
        groups.setdefault((e[0], e[1], e[2], len(e[3]), e[4]), []).append(e)
    rest = [e for e in uniq if len(groups[(e[0], e[1], e[2], len(e[3]), e[4])]) == 1]
    rest.sort(key=lambda e: (e[2] + len(e[3]), -e[4], e[0], e[1], e[2], e[3]))
    taken, accepted, nconf = {}, [], 0
    for e in rest:
        lst = taken.setdefault(e[0], [])
        key = (e[1], e[1] + e[2])
        i = bisect.bisect_left(lst, key)
        clash = (i < len(lst) and lst[i][0] - key[1] < k - 1) or (i > 0 and key[0] - lst[i - 1][1] < k - 1)
        if clash:
            nconf += 1
        else:
            lst.insert(i, key)
            accepted.append(e)
    accepted.sort(key=lambda e: (e[0], e[1]))
    return accepted, len(uniq), nconf, len(uniq) - len(rest)


def select_plain(edits, k):
    """the same straight from the rule: every pair looked at"""
    uniq = []
    for e in edits:
        if not any(u[:4] == e[:4] for u in uniq):
            uniq.append(e)
    amb = [e for e in uniq if any(o[:3] == e[:3] and len(o[3]) == len(e[3]) and o[4] == e[4] and o[3] != e[3] for o in uniq)]
    rest = sorted((e for e in uniq if e not in amb), key=lambda e: (e[2] + len(e[3]), -e[4], e[0], e[1], e[2], e[3]))
    accepted, nconf = [], 0
    for e in rest:
        if any(conflicts(a, e, k) for a in accepted):
            nconf += 1
        else:
            accepted.append(e)
    return sorted(accepted, key=lambda e: (e[0], e[1])), len(uniq), nconf, len(amb)


def apply_edits(seqs, edits):
    """plain slicing; edits (seq, pos, rlen, y, ...) -> list of bytes"""
    out = [bytearray(as_bytes(s)) for s in seqs]
    for e in sorted(edits, key=lambda e: (e[0], e[1]), reverse=True):
        out[e[0]][e[1]:e[1] + e[2]] = as_bytes(e[3])
    return [bytes(b) for b in out]


def report_of(seqs, k, count, thre):
    return restate_runs([window_counts(s, k, count) for s in seqs], thre)


def restate_repair(seqs, k, count, thre, indel_max_len=4, compound_max_len=64, rounds=3):
    """dict: seqs (bytes), edits [(round, seq, pos, rlen, y, source, ref_min, alt_min)] in (round, seq, pos) order, rounds [(records,
    accepted, conflicts, ambiguous, unreliable_before, unreliable_after)], before / after ((counts, runs) of the report), texts (the
    sequences before round 1, 2, .. and at the end)"""
    cur = [as_bytes(s) for s in seqs]
    res = dict(edits=[], rounds=[], texts=[cur], before=None, after=None)
    settled = False
    for r in range(1, rounds + 1):
        rep = report_of(cur, k, count, thre)
        unrel = sum(c[2] for c in rep[0])
        if r == 1:
            res["before"] = rep
        else:
            res["rounds"][-1] = res["rounds"][-1][:5] + (unrel,)
        edits = normalise(restate_variants(cur, k, count, thre)[1], restate_indels(cur, k, count, thre, indel_max_len)[1],
                          restate_mixed(cur, k, count, thre, indel_max_len)[1], restate_compound(cur, k, count, thre, compound_max_len)[1])
        acc, nrec, nconf, namb = select(edits, k)
        res["rounds"].append((nrec, len(acc), nconf, namb, unrel, unrel))
        if not acc:
            res["after"] = rep
            settled = True
            break
        res["edits"] += [(r, e[0], e[1], e[2], e[3], e[6], e[5], e[4]) for e in acc]
        cur = apply_edits(cur, acc)
        res["texts"].append(cur)
    if not settled:
        res["after"] = report_of(cur, k, count, thre)
        res["rounds"][-1] = res["rounds"][-1][:5] + (sum(c[2] for c in res["after"][0]),)
    res["seqs"] = cur
    return res


def texts_of(seqs, edit_tuples):
    """the sequences before round 1, 2, .. and at the end, from the input and a result's edits (round, seq, pos, rlen, y, ...)"""
    texts = [[as_bytes(s) for s in seqs]]
    for r in sorted({e[0] for e in edit_tuples}):
        texts.append(apply_edits(texts[-1], [e[1:] for e in edit_tuples if e[0] == r]))
    return texts


def check_invariants(texts, edit_tuples, round_tuples, k, count, thre):
    """per accepting round: unreliable_after == unreliable_before - the unreliable windows w of the old text with pos-k+1 <= w < pos+rlen
    (for rlen = 0: w < pos), clipped, summed over the edits; that is >= 1 per edit; and no unreliable window of the new text overlaps an
    applied y or spans an applied deletion's junction"""
    for ri, rt in enumerate(round_tuples):
        mine = [e for e in edit_tuples if e[0] == ri + 1]
        assert len(mine) == rt[1]
        if not mine:
            assert rt[4] == rt[5]
            continue
        old = [[c is not None and c < thre for c in window_counts(s, k, count)] for s in texts[ri]]
        new = [[c is not None and c < thre for c in window_counts(s, k, count)] for s in texts[ri + 1]]
        assert rt[4] == sum(sum(u) for u in old) and rt[5] == sum(sum(u) for u in new)
        gone, shift, last = 0, 0, -1
        for _r, seq, pos, rlen, y, *_ in mine:          # (in (seq, pos) order)
            if seq != last:
                shift, last = 0, seq
            u = old[seq]
            n = sum(u[max(0, pos - k + 1):max(0, min(len(u), pos + rlen))])
            assert n >= 1, (ri + 1, seq, pos)
            gone += n
            p2 = pos + shift                            # where y starts in the new text
            v = new[seq]
            assert not any(v[max(0, p2 - k + 1):max(0, min(len(v), p2 + len(y)))]), (ri + 1, seq, pos)
            shift += len(y) - rlen
        assert rt[5] == rt[4] - gone, (ri + 1, rt, gone)


def summary(res):
    """[(accepted, conflicts, ambiguous, {source: n}, unreliable_before, unreliable_after)] of the accepting rounds"""
    out = []
    for ri, rt in enumerate(res["rounds"]):
        if rt[1]:
            src = {}
            for e in res["edits"]:
                if e[0] == ri + 1:
                    src[e[5]] = src.get(e[5], 0) + 1
            out.append((rt[1], rt[2], rt[3], src, rt[4], rt[5]))
    return out


@functools.lru_cache(maxsize=None)
def golden_repair(name, rounds=3):
    """(case, sequences, count, restate_repair of them) of a golden case, computed once for all tests of a run"""
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    return c, seqs, count, restate_repair(seqs, c.k, count, c.thre, 4, 64, rounds)


@functools.lru_cache(maxsize=None)
def pairs_repair(k):
    truth, contig, pairs, far = planted_pairs(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    return truth, contig, pairs, far, count, restate_repair([contig], k, count, 3, 4, 64, 3)


FUZZ = [(k, seed, thre) for k in (5, 6, 7) for seed in range(400, 420) for thre in (1, 2)]


@functools.lru_cache(maxsize=None)
def fuzz_repair(k, seed, thre):
    reads, seqs = tiny_fuzz(k, seed)
    count = dict_counter(kmer_dict(reads, k))
    return reads, seqs, count, restate_repair(seqs, k, count, thre, 4, 8, 3)


# ---- anchors on the committed dumps ----------------------------------------------------------------------------------------------
# per accepting round (accepted, conflicts, unreliable before, unreliable after); no ambiguity anywhere
ANCHORS = {"cluster_k25": [(12, 1, 450, 68), (1, 0, 68, 19)], "cluster_k37": [(11, 0, 599, 31)], "diploid_k25": [(3, 0, 103, 14)], "edges_k19": [(7, 0, 168, 39)],
           "edges_k25": [(7, 0, 219, 48)], "gaps_k25": [(30, 0, 1280, 467)], "gaps_k37_p4": [(31, 0, 1779, 575)], "homopolymer_k21": [(10, 0, 169, 26)],
           "homopolymer_k25": [(10, 0, 212, 27)], "rolling_k25": [(3, 0, 112, 40)], "rolling_k37": [(3, 0, 156, 46)], "simple_k17_p1": [(9, 0, 165, 17)],
           "simple_k25": [(9, 0, 242, 21)], "simple_k31_p3": [(9, 0, 288, 15)], "simple_k37": [(9, 0, 364, 41)], "simple_k45": [(9, 0, 435, 35)],
           "simple_k63": [(9, 0, 575, 13)]}
SOURCE_ANCHORS = {"cluster_k25": [dict(compound=7, sub=4, ins=1), dict(compound=1)], "gaps_k25": [{"ins": 7, "sub": 5, "compound": 5, "del": 13}],
                  "homopolymer_k21": [{"del": 6, "ins": 3, "mixed": 1}]}


def test_the_anchors_name_golden_cases():
    assert set(ANCHORS) == set(case_names()) and len(case_names()) == 17


@pytest.mark.parametrize("name", case_names())
def test_golden_anchors(name):
    c, seqs, count, res = golden_repair(name)
    got = summary(res)
    assert [(a, cf, ub, ua) for a, cf, _amb, _src, ub, ua in got] == ANCHORS[name], (name, res["rounds"])
    assert all(g[2] == 0 for g in got) and all(rt[3] == 0 for rt in res["rounds"])
    if name in SOURCE_ANCHORS:
        assert [g[3] for g in got] == SOURCE_ANCHORS[name]
    if name == "cluster_k25":
        assert res["rounds"][0][0] == 13 and res["rounds"][1][0] == 1
    assert res["rounds"][-1][1] == 0 and len(res["rounds"]) == len(got) + 1      # the loop ended on a round that accepted nothing
    assert res["texts"] == texts_of(seqs, res["edits"])
    check_invariants(res["texts"], res["edits"], res["rounds"], c.k, count, c.thre)
    assert res["before"][0] == report_of(seqs, c.k, count, c.thre)[0] and res["after"] == report_of(res["seqs"], c.k, count, c.thre)


def test_one_round_stops_there_and_reports_once_more():
    c, seqs, count, res = golden_repair("cluster_k25", 1)
    assert res["rounds"] == [(13, 12, 1, 0, 450, 68)] and len(res["edits"]) == 12
    assert res["after"] == report_of(res["seqs"], c.k, count, c.thre) and res["seqs"] == golden_repair("cluster_k25")[3]["texts"][1]


@pytest.mark.parametrize("k", [21, 31])
def test_planted_pairs(k):
    """reads = 5 copies of the truth, thre 3: 11 records, 10 applied, one conflict -- the compound record over the pair k apart loses to
    the two substitutions it spans; the repaired text is the truth"""
    truth, contig, pairs, far, count, res = pairs_repair(k)
    assert res["rounds"][0][:4] == (11, 10, 1, 0) and [rt[1] for rt in res["rounds"]] == [10, 0]
    assert res["seqs"] == [truth] and res["rounds"][0][5] == 0 and res["rounds"][1][4:] == (0, 0)
    p, d = pairs[-1]
    assert d == k and sorted(e[2] for e in res["edits"] if e[5] == "sub") == sorted([p, p + k, far[0], far[1]])
    assert not any(e[2] == p and e[5] == "compound" for e in res["edits"])
    check_invariants(res["texts"], res["edits"], res["rounds"], k, count, 3)


def test_tiny_fuzz():
    seen = dict(inputs=0, two_rounds=0, conflicts=0, edits=0)
    for k, seed, thre in FUZZ:
        reads, seqs, count, res = fuzz_repair(k, seed, thre)
        check_invariants(res["texts"], res["edits"], res["rounds"], k, count, thre)
        assert res["texts"] == texts_of(seqs, res["edits"])
        us = [rt[4] for rt in res["rounds"]]
        assert all(a > b for a, b in zip(us, us[1:])) or len(us) == 1      # every accepting round strictly lowers the unreliable windows
        seen["inputs"] += 1
        seen["two_rounds"] += sum(1 for rt in res["rounds"] if rt[1]) >= 2
        seen["conflicts"] += sum(rt[2] for rt in res["rounds"])
        seen["edits"] += len(res["edits"])
    assert seen["two_rounds"] >= 1 and seen["conflicts"] >= 1 and seen["edits"] > 100, seen
    two = {seed for k, seed, thre in FUZZ if k == 7 and sum(1 for rt in fuzz_repair(k, seed, thre)[3]["rounds"] if rt[1]) >= 2}
    assert {401, 408, 418} <= two, two


# ---- the selection -----------------------------------------------------------------------------------------------------------------
def E(seq, pos, rlen, y, amin=5, source="compound"):
    return (seq, pos, rlen, y, amin, 0, source)


def test_selection_on_hand_made_edits():
    k = 5
    acc, nrec, nconf, namb = select([E(0, 100, 1, "G", 5, "sub"), E(0, 103, 3, "ACG", 9), E(0, 109, 1, "T", 5, "sub"), E(0, 200, 2, "AC", 3), E(0, 203, 2, "GT", 4)], k)
    assert ([e[1] for e in acc], nrec, nconf, namb) == ([100, 109, 203], 5, 2, 0)
    # exactly k - 1 apart is no conflict; an insertion has q = pos
    acc, _, nconf, _ = select([E(0, 10, 1, "A"), E(0, 15, 0, "CC"), E(0, 19, 2, ""), E(0, 24, 1, "T")], k)
    assert [e[1] for e in acc] == [10, 15, 19] and nconf == 1
    # nesting
    acc, _, nconf, _ = select([E(0, 50, 20, "ACGTACGTAC"), E(0, 58, 1, "G", 5, "sub"), E(0, 58, 1, "GA")], k)
    assert [e[6] for e in acc] == ["sub"] and nconf == 2
    # ambiguity: same place, lengths and alt_min, another y: both go; a duplicate is one edit, the first source stays
    acc, nrec, nconf, namb = select([E(0, 30, 2, "AC"), E(0, 30, 2, "AG"), E(0, 30, 2, "TT", 6), E(1, 30, 2, "AC", 5, "mixed"), E(1, 30, 2, "AC")], k)
    assert (nrec, nconf, namb) == (4, 0, 2) and [(e[0], e[3], e[6]) for e in acc] == [(0, "TT", "compound"), (1, "AC", "mixed")]
    # all ambiguous: nothing is accepted
    assert select([E(0, 30, 0, "A"), E(0, 30, 0, "C")], k) == ([], 2, 0, 2)
    # two sequences do not see each other
    acc, _, nconf, _ = select([E(0, 10, 1, "A"), E(1, 10, 1, "A"), E(1, 11, 1, "C"), E(2, 0, 0, "G")], k)
    assert [(e[0], e[1]) for e in acc] == [(0, 10), (1, 10), (2, 0)] and nconf == 1


def test_the_selection_agrees_with_its_plain_form():
    import numpy as np
    rng = np.random.default_rng(5)
    seen = dict(conflicts=0, ambiguous=0, dups=0)
    for _ in range(300):
        k = int(rng.integers(2, 12))
        edits = []
        for _i in range(int(rng.integers(1, 60))):
            y = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 4))))
            rlen = int(rng.integers(0, 4))
            if not y and not rlen:
                y = "C"
            edits.append(E(int(rng.integers(0, 2)), int(rng.integers(0, 80)), rlen, y, int(rng.integers(3, 6)), SOURCES[int(rng.integers(0, 5))]))
        got = select(edits, k)
        assert got == select_plain(edits, k)
        assert got[1] == len(got[0]) + got[2] + got[3]
        seen["conflicts"] += got[2]
        seen["ambiguous"] += got[3]
        seen["dups"] += len(edits) - got[1]
    assert min(seen.values()) > 0, seen
    for k, seed, thre in FUZZ[::7]:                     # and on what the scans give
        reads, seqs, count, _ = fuzz_repair(k, seed, thre)
        edits = normalise(restate_variants(seqs, k, count, thre)[1], restate_indels(seqs, k, count, thre, 4)[1], restate_mixed(seqs, k, count, thre, 4)[1],
                          restate_compound(seqs, k, count, thre, 8)[1])
        assert select(edits, k) == select_plain(edits, k)


# ---- writers ---------------------------------------------------------------------------------------------------------------------
def test_writer_texts():
    from jasper_amd import repair
    polished = ["GATTacaTCAGAGAGCTN", "ACGTACGTAC", ""]
    # (round, seq, pos, rlen, y, source, ref_min, alt_min): c2 has no edit
    edits = [(2, 0, 1, 0, "CC", "ins", 1, 6), (1, 0, 4, 3, "GT", "compound", 0, 7), (1, 0, 13, 1, "", "del", 2, 4), (1, 0, 0, 1, "C", "sub", 0, 9)]
    round1 = ["CATTGTTCAGAGGCTN", "ACGTACGTAC", ""]
    final = ["CCCATTGTTCAGAGGCTN", "ACGTACGTAC", ""]
    assert [apply_edits(polished, [e[1:] for e in edits if e[0] == 1]), apply_edits(round1, [e[1:] for e in edits if e[0] == 2])] == [
        [s.encode() for s in round1], [s.encode() for s in final]]
    # the FASTA: header lines as they stand, a contig without an edit byte for byte (here on two lines), a header without a sequence kept
    fasta = ">c1 first\n%s\n>c0 empty\n>c00 an empty line\n\n>c2\nACGTAC\nGTAC\n" % polished[0]
    assert repair.fasta_text(fasta, final[:2]) == ">c1 first\nCCCATTGTTCAGAGGCTN\n>c0 empty\n>c00 an empty line\n\n>c2\nACGTAC\nGTAC\n"
    assert repair.fasta_text(fasta, [polished[0].encode(), b"ACGTACGTAC"]) == fasta
    with pytest.raises(ValueError):
        repair.fasta_text(fasta, final)
    assert repair.round_texts(polished, edits) == [polished, round1]
    assert repair.repairs_tsv_text(["c1", "c2", "c3"], [polished, round1], edits) == (
        "#round\tcontig\tpos\tref\talt\tsource\trc\tac\n"
        "1\tc1\t0\tG\tC\tsub\t0\t9\n1\tc1\t4\taca\tGT\tcompound\t0\t7\n1\tc1\t13\tA\t.\tdel\t2\t4\n2\tc1\t1\t.\tCC\tins\t1\t6\n")
    before = [(14, 10, 4, 1), (6, 6, 0, 0), (0, 0, 0, 0)]
    after = [(14, 13, 1, 0), (6, 6, 0, 0), (0, 0, 0, 0)]
    assert repair.repair_tsv_text(5, ["c1", "c2", "c3"], [18, 10, 0], [18, 10, 0], edits, before, after) == (
        "#contig\tlength_polished\tlength_repaired\tsub\tins\tdel\tmixed\tcompound\tvalid_before\tunreliable_before\tQV_before\tvalid_after\tunreliable_after\tQV_after\n"
        "c1\t18\t18\t1\t1\t1\t0\t1\t10\t4\t%s\t13\t1\t%s\n"
        "c2\t10\t10\t0\t0\t0\t0\t0\t6\t0\tinf\t6\t0\tinf\n"
        "c3\t0\t0\t0\t0\t0\t0\t0\t0\t0\tNA\t0\t0\tNA\n"
        "*\t28\t28\t1\t1\t1\t0\t1\t16\t4\t%s\t19\t1\t%s\n" % (qv(4, 10, 5), qv(1, 13, 5), qv(4, 16, 5), qv(1, 19, 5)))
    assert repair.log_text(5, [(5, 3, 1, 1, 4, 2), (2, 1, 0, 1, 2, 1), (1, 0, 0, 1, 1, 1)], before, after) == (
        "Repair: round 1: 5 records, 3 accepted, 1 conflicts, 1 ambiguous; round 2: 2 records, 1 accepted, 0 conflicts, 1 ambiguous; "
        "round 3: 1 records, 0 accepted, 0 conflicts, 1 ambiguous; unreliable kmers 4 -> 1, dense QV %s -> %s" % (qv(4, 16, 5), qv(1, 19, 5)))
    # no edit at all
    assert repair.repairs_tsv_text(["c1"], [["ACGT"]], []) == "#round\tcontig\tpos\tref\talt\tsource\trc\tac\n"


def qv(x, valid, k):
    """the report's formula (jasper_amd/report.py, src/jasper.sh:239-242), restated"""
    import math
    if valid <= 0:
        return "NA"
    if x <= 0:
        return "inf"
    return "%.4f" % (-10.0 * math.log10(1.0 - (1.0 - x / valid) ** (1.0 / k)) + 0.0)


def test_files_are_written_through_a_rename(tmp_path):
    from jasper_amd import repair
    repair.write_atomic(str(tmp_path / "x.tsv"), "a\n")
    assert [f.name for f in tmp_path.iterdir()] == ["x.tsv"] and (tmp_path / "x.tsv").read_text() == "a\n"


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    return subprocess.run([sys.executable, "-m", "jasper_amd.cli"] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)


def _inputs(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "r.fa"
    fq.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    return ["-a", str(fa), "-r", str(fq), "-k", "5"]


@pytest.mark.parametrize("bad", ["0", "9", "-1", "x", "2.5"])
def test_a_bad_number_of_rounds_ends_the_run(bad, tmp_path):
    r = _run(_inputs(tmp_path) + ["--repair", "--repair-rounds", bad], tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--repair-rounds takes an integer from 1 to 8; it is %s" % bad in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


def test_rounds_without_repair_end_the_run(tmp_path):
    r = _run(_inputs(tmp_path) + ["--repair-rounds", "2"], tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--repair-rounds needs --repair" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


@pytest.mark.parametrize("flag, bad, msg", [("--indel-max-len", "17", "--indel-max-len takes an integer from 1 to 16; it is 17"),
                                            ("--compound-max-len", "65", "--compound-max-len takes an integer from 1 to 64; it is 65")])
def test_repair_honours_the_scans_lengths(flag, bad, msg, tmp_path):
    """--repair needs neither --indels nor --compound, but takes their lengths: a bad one ends the run before anything is counted"""
    r = _run(_inputs(tmp_path) + ["--repair", flag, bad], tmp_path)
    assert r.returncode == 1 and msg in r.stdout + r.stderr, (r.stdout, r.stderr)
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


def test_threshold_zero_ends_the_driver(capsys):
    from jasper_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.run_repair(None, [(">c", "ACGT")], 0, 4, 64, 3)
    assert e.value.code == 1
    out = capsys.readouterr()
    assert "--repair needs a threshold for unreliable kmers of at least 1; it is 0" in out.out + out.err
    assert cli.repair_flags(False, None) == 0 and cli.repair_flags(True, None) == 3 and cli.repair_flags(True, "8") == 8


# ---- the C++ selection under sanitizers --------------------------------------------------------------------------------------------
def test_host_check_program_under_sanitizers(tmp_path):
    """tools/repair_host_check.cpp: normalisation, selection (priority, chains, nesting, ambiguity, two sequences), the plan and
    check_edits of jasper_amd/csrc/repair_host.hpp as a stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "repair_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "repair_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
