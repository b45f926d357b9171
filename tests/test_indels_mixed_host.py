"""CPU: the mixed half of the indel scan.  The restatement of its semantics that the GPU tests compare against (test_gpu_indels_mixed.py,
test_gpu_cli_indels_mixed.py), checked here against a plain form by enumeration and on the committed dumps of the golden cases; and
the host side (jasper_amd/indels.py: rotation to the left, the three TSV columns, the VCF lines, the log texts; --indel-mixed without
--indels) on hand-made records.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h, jasper_indel_scan_mixed): s of n bytes, case folded; F = s[p-k+1 .. p-1]; cnt = the count of a canonical
k-mer, clamped to 2^32-1; FRONT = 64.
  ins(p, y), y of L bases, 1 <= L <= max_len <= 16, y[0] != s[p]: evaluated iff k-1 <= p <= n-k+1 and s[p-k+1 .. p+k-2] are all bases;
      its alternative string is F + y + s[p .. p+k-2], of k+L-1 windows
  the search at (p, x), evaluated and with cnt(F + x) >= thre: S_1 = {x}; S_t = {yz : y in S_(t-1), z in ACGT, cnt(the last k bytes of
      F + y + z) >= thre}.  It runs t = 1, 2, .. and ends at the first of: t > max_len, S_t empty, |S_t| > FRONT -- then the site is
      complex, counted once per (p, x), and nothing of length >= t is reported there
  a record (seq, p, t, y, ref_min, alt_min, kind) for every y in S_t of a level that was reached, y != x^t, whose windows t .. k+t-2 of
      the alternative string are >= thre too; alt_min over all k+t-1 windows; ref_min over the k-1 windows of s that start at
      p-k+1 .. p-1; kind 1 (het) when ref_min >= thre, else 2
  ordered by (seq, pos, len, y); per sequence (mixed_het, mixed_error, complex)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import Case, case_names
from test_gpu_copies import as_bytes, dict_counter, kmer_dict
from test_indels_host import ACGT, ERROR, HET, U32, plant, rand_bases, restate

FRONT = 64


def _finish(recs, n_seqs, complex_):
    recs.sort(key=lambda r: (r[0], r[1], r[2], r[3]))
    counts = [[0, 0, c] for c in complex_]
    for r in recs:
        counts[r[0]][r[6] - 1] += 1
    return [tuple(c) for c in counts], recs


def restate_mixed(seqs, k, count, thre, max_len, stats=None, same_base=False):
    """(counts, records) of the semantics above; count(bytes of k upper-case bases) -> int.  Shortcuts: the frontier is carried from
    level to level with its running minimum, the rejoin windows stop at the first one below thre, ref_min is computed once per
    position.  stats, a dict, gets `candidates`, `complex`, `widest` (the largest level that was searched), `levels` (the sizes of all
    levels t >= 2 that were computed, those above FRONT too) and `same_base` (solid insertions x^t, which are not records).
    same_base=True lists those as records too (for comparison with the same-base scan)."""
    recs, complex_ = [], [0] * len(seqs)
    st = dict(candidates=0, complex=0, widest=0, levels=[], same_base=0)
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        n = len(up)
        pre = [0] * (n + 1)
        for i, ch in enumerate(up):
            pre[i + 1] = pre[i] + (0 if ch in ACGT else 1)
        for p in range(k - 1, n - k + 2):
            if pre[p + k - 1] != pre[p - k + 1]:
                continue
            F, tail = up[p - k + 1:p], up[p:p + k - 1]
            rmin = None
            for x in ACGT:
                xb = bytes([x])
                c0 = min(count(F + xb), U32)
                if x == up[p] or c0 < thre:
                    continue
                st["candidates"] += 1
                S, t = [(xb, c0)], 1
                while True:
                    st["widest"] = max(st["widest"], len(S))
                    for y, m in S:
                        alt = (F + y + tail)[t:]                      # windows t .. k+t-2
                        amin = m
                        for j in range(k - 1):
                            amin = min(amin, min(count(alt[j:j + k]), U32))
                            if amin < thre:
                                break
                        if amin < thre:
                            continue
                        if y == xb * t:
                            st["same_base"] += 1
                            if not same_base:
                                continue
                        if rmin is None:
                            rmin = min(min(count(up[j:j + k]), U32) for j in range(p - k + 1, p))
                        recs.append((si, p, t, y.decode(), rmin, amin, HET if rmin >= thre else ERROR))
                    if t == max_len:
                        break
                    new = []
                    for y, m in S:
                        for z in ACGT:
                            c = min(count((F + y + bytes([z]))[-k:]), U32)
                            if c >= thre:
                                new.append((y + bytes([z]), min(m, c)))
                    st["levels"].append(len(new))
                    if len(new) > FRONT:
                        complex_[si] += 1
                        st["complex"] += 1
                        break
                    if not new:
                        break
                    S, t = new, t + 1
    if stats is not None:
        stats.update(st)
    return _finish(recs, len(seqs), complex_)


def restate_mixed_plain(seqs, k, count, thre, max_len):
    """the same straight from the definition: every p, every string y of every length, every minimum over all its windows; the level
    sizes |S_t| computed separately, as the number of strings of length t that start with x and have t solid windows"""
    recs, complex_ = [], [0] * len(seqs)
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        n = len(up)

        def cmin(a):
            return min(min(count(a[j:j + k]), U32) for j in range(len(a) - k + 1))

        for p in range(n):
            if not (k - 1 <= p <= n - k + 1 and all(ch in ACGT for ch in up[p - k + 1:p + k - 1])):
                continue
            F, tail = up[p - k + 1:p], up[p:p + k - 1]
            rmin = cmin(up[p - k + 1:p + k - 1])
            for x in ACGT:
                xb = bytes([x])
                if x == up[p]:
                    continue
                size = {}
                for t in range(1, max_len + 1):
                    size[t] = sum(1 for rest in itertools.product(ACGT, repeat=t - 1) if cmin(F + xb + bytes(rest)) >= thre)
                reached = 0                                   # the levels 1 .. reached are searched
                for t in range(1, max_len + 1):
                    if size[t] == 0:
                        break
                    if size[t] > FRONT:
                        complex_[si] += 1
                        break
                    reached = t
                for t in range(1, reached + 1):
                    for rest in itertools.product(ACGT, repeat=t - 1):
                        y = xb + bytes(rest)
                        if y == xb * t:
                            continue
                        amin = cmin(F + y + tail)
                        if amin >= thre:
                            recs.append((si, p, t, y.decode(), rmin, amin, HET if rmin >= thre else ERROR))
    return _finish(recs, len(seqs), complex_)


def random_string(rng, L, not_first=None):
    """L random bases; the first one is not the byte not_first"""
    while True:
        y = rand_bases(rng, L)
        if not_first is None or y[0] != not_first:
            return y


def plant_strings(h, events):
    """h with events [(q, 'ins', y) | (q, 'del', L)] applied (positions in h, ascending) -> the other haplotype"""
    out, at = [], 0
    for q, typ, v in events:
        out.append(h[at:q])
        if typ == "ins":
            out.append(v)
            at = q
        else:
            at = q + v
    out.append(h[at:])
    return b"".join(out)


def right_most(s, q, y):
    """the insertion of y before s[q] at its right-most position: while s[q] == y[0], y[1:] + y[0] before q + 1"""
    while q < len(s) and s[q] == y[0]:
        y = y[1:] + y[:1]
        q += 1
    return q, y


def left_most(s, q, y):
    """the rule of the VCF writer, restated: while q > 1 and s[q-1] == y[-1], y[-1] + y[:-1] before q - 1"""
    while q > 1 and s[q - 1] == y[-1]:
        y = y[-1:] + y[:-1]
        q -= 1
    return q, y


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def tiny_fuzz(k, seed=91):
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, 120)
    g2 = plant_strings(g, [(30, "ins", b"GAT" if g[30] != ord("G") else b"CAT"), (60, "del", 2), (90, "ins", b"TC" if g[90] != ord("T") else b"AC")])
    a = bytearray(g)
    a[75] = ord("N")
    a[100:110] = bytes(a[100:110]).lower()
    return [g] * 2 + [g2] * 2, [bytes(a), g[:2 * k - 3], g[:2 * k - 2], g[10:10 + 2 * k - 1], b"", g2[20:70]]


def test_the_restatement_agrees_with_its_plain_form():
    seen_complex = 0
    for k in (2, 3, 5):
        reads, seqs = tiny_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        for thre, max_len in ((1, 1), (1, 5), (2, 4), (3, 5)):
            got = restate_mixed(seqs, k, count, thre, max_len)
            assert got == restate_mixed_plain(seqs, k, count, thre, max_len), (k, thre, max_len)
            seen_complex += sum(c[2] for c in got[0])
            if max_len > 1 and thre < 3:
                assert len(got[1]) > 20
    assert seen_complex > 0                                  # at k = 2 nearly every string is solid: 256 prefixes of length 5


def test_same_base_strings_are_the_same_base_scan():
    """with the same-base strings listed too, those of the mixed restatement are the insertions of test_indels_host.restate, where no
    site is complex"""
    for k, max_len in ((3, 3), (4, 4)):                     # (at most 4^(max_len - 1) <= 64 prefixes: no level is cut)
        reads, seqs = tiny_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        st = {}
        _, recs = restate_mixed(seqs, k, count, 1, max_len, st, same_base=True)
        assert st["complex"] == 0
        same = [(r[0], r[1], r[2], r[3][0], r[4], r[5], r[6]) for r in recs if r[3] == r[3][0] * r[2]]
        ins = [(r[0], r[1], r[3], r[4], r[5], r[6], r[7]) for r in restate(seqs, k, count, 1, max_len)[1] if r[2] == "ins"]
        assert sorted(same) == sorted(ins) and len(ins) > 0 and st["same_base"] == len(ins)


def two_haplotypes(seed=2031, n=6000):
    """the planted pair of the issue: 6000 random bases, 12 insertions of random strings and 12 deletions, lengths 1..16, 220 bytes
    apart; reads: 6 copies of h1, 5 of h2 -> (h1, h2, reads, events)"""
    rng = np.random.default_rng(seed)
    h1 = rand_bases(rng, n)
    events = []
    for i in range(24):
        q = 300 + 220 * i + int(rng.integers(0, 20))
        L = (1, 2, 3, 4, 5, 8, 16, 7, 11, 13, 6, 9)[i // 2]
        events.append((q, "ins", random_string(rng, L)) if i % 2 == 0 else (q, "del", L))
    h2 = plant_strings(h1, events)
    return h1, h2, [h1] * 6 + [h2] * 5, events


def views(h1, h2, events):
    """what each side must list for the events: from h1, h2's insertions; from h2, h1's deleted bytes as insertions -- each at its
    right-most position, [(pos, len, y)] without the same-base strings, which are the same-base scan's"""
    from1, from2, shift = [], [], 0
    for q, typ, v in events:
        if typ == "ins":
            from1.append(right_most(h1, q, v))
            shift += len(v)
        else:
            from2.append(right_most(h2, q + shift, h1[q:q + v]))
            shift -= v
    keep = lambda lst: sorted((q, len(y), y.decode()) for q, y in lst if y != y[:1] * len(y))      # noqa: E731
    return keep(from1), keep(from2)


@pytest.mark.parametrize("k", [31, 64])
def test_both_sides_of_one_pair(k):
    h1, h2, reads, events = two_haplotypes()
    count = dict_counter(kmer_dict(reads, k))
    want1, want2 = views(h1, h2, events)
    assert len(want1) >= 10 and len(want2) >= 10
    got1 = restate_mixed([h1], k, count, 3, 16)
    got2 = restate_mixed([h2], k, count, 3, 16)
    assert [(r[1], r[2], r[3]) for r in got1[1]] == want1 and [(r[1], r[2], r[3]) for r in got2[1]] == want2
    assert all(r[4:] == (6, 5, HET) for r in got1[1]) and all(r[4:] == (5, 6, HET) for r in got2[1])
    assert got1[0] == [(len(want1), 0, 0)] and got2[0] == [(len(want2), 0, 0)]


# ---- anchors on the committed dumps ----------------------------------------------------------------------------------------------
MIXED_ANCHORS = {"homopolymer_k21": 1, "homopolymer_k25": 1}          # mixed records; 0 in every other case
WIDEST = {"rolling_k25": 7, "rolling_k37": 9}                         # the widest level; 1 in every other case


@pytest.mark.parametrize("name", case_names())
def test_golden_anchors(name):
    import test_gpu_indels
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    for max_len in (4, 16):
        st = {}
        counts, recs = restate_mixed(seqs, c.k, count, c.thre, max_len, st)
        assert len(recs) == MIXED_ANCHORS.get(name, 0), (name, max_len, recs)
        assert st["widest"] == (WIDEST.get(name, 1) if st["candidates"] else 0), (name, max_len, st["widest"])
        assert st["complex"] == 0 and all(c3[2] == 0 for c3 in counts)
        n_ins = sum(r[2] == "ins" for r in restate(seqs, c.k, count, c.thre, max_len)[1])
        assert st["same_base"] == n_ins
        if max_len == 4 and name in test_gpu_indels.ANCHORS:
            assert st["same_base"] == test_gpu_indels.ANCHORS[name][0]


def test_the_anchors_name_golden_cases():
    assert set(MIXED_ANCHORS) | set(WIDEST) <= set(case_names()) and len(case_names()) == 17


# ---- writers ---------------------------------------------------------------------------------------------------------------------
def test_left_align_by_rotation():
    from jasper_amd.indels import left_align_mixed
    #    0123456789012
    s = "GATCACACGTTAN"
    assert left_align_mixed(s, 8, "AC") == (3, "CA")           # ..ACAC|G + AC: rotates through the tandem copies to T|CA
    assert left_align_mixed(s, 8, "TC") == (7, "CT")           # one step: s[7] == 'C'
    assert left_align_mixed(s, 8, "GA") == (8, "GA")
    assert left_align_mixed(s, 11, "ATT") == (9, "TTA")
    assert left_align_mixed("ACAC", 4, "AC") == (1, "CA")      # q = 1 stops it: the anchor is byte 0
    assert left_align_mixed("GNCAC", 5, "AC") == (2, "CA")     # an N stops it
    assert left_align_mixed("gtcacacg", 7, "ac") == (2, "CA") and left_align_mixed(b"GTCACACG", 7, "AC") == (2, "CA")
    for q, y in ((8, "AC"), (8, "TC"), (11, "ATT"), (5, "GGC")):
        assert left_align_mixed(s, q, y) == tuple(v if isinstance(v, int) else v.decode() for v in left_most(s.encode(), q, y.encode()))


def test_tsv_columns():
    from jasper_amd import indels
    names = ["c1", "c2"]
    plain = [("before", [100, 50], [(1, 2, 3, 4), (0, 0, 1, 0)]), ("after", [99, 50], [(1, 0, 3, 0), None])]
    mixed = [plain[0] + ([(5, 6, 7), (0, 1, 0)],), plain[1] + ([(2, 0, 1), None],)]
    assert indels.indels_tsv_text(names, mixed) == (
        "#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error\tmixed_het\tmixed_error\tcomplex\n"
        "c1\tbefore\t100\t1\t2\t3\t4\t5\t6\t7\nc1\tafter\t99\t1\t0\t3\t0\t2\t0\t1\n"
        "c2\tbefore\t50\t0\t0\t1\t0\t0\t1\t0\nc2\tafter\t0\t0\t0\t0\t0\t0\t0\t0\n"
        "*\tbefore\t150\t1\t2\t4\t4\t5\t7\t7\n*\tafter\t99\t1\t0\t3\t0\t2\t0\t1\n")
    # without the mixed half every byte is what it was
    assert indels.indels_tsv_text(names, plain) == ("#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error\n"
                                                    "c1\tbefore\t100\t1\t2\t3\t4\nc1\tafter\t99\t1\t0\t3\t0\n"
                                                    "c2\tbefore\t50\t0\t0\t1\t0\nc2\tafter\t0\t0\t0\t0\t0\n"
                                                    "*\tbefore\t150\t1\t2\t4\t4\n*\tafter\t99\t1\t0\t3\t0\n")
    assert indels.mixed_stage_log_text([(5, 6, 7), (0, 1, 0)]) == "5 het and 7 error mixed insertions, 7 complex sites"
    assert indels.mixed_log_text([(5, 6, 7)], [(2, 0, 1), None]) == ("Mixed insertions: before polishing 5 het and 6 error mixed insertions, 7 complex sites; "
                                                                     "after polishing 2 het and 0 error mixed insertions, 1 complex sites")


def test_vcf_text_with_mixed_lines():
    from jasper_amd import indels
    from jasper_amd.table import MIXED_DTYPE
    names, seqs = ["c1", "c2"], ["GATTTTTCAGAGAGCTN", "ACGTACGTAC"]
    recs = [(0, 6, "del", 1, "C", 6, 5, 1),                    # c1: POS 2, REF AT ALT A
            (0, 7, "ins", 1, "T", 6, 4, 1),                    # c1: POS 2, REF A ALT AT
            (0, 7, "ins", 2, "T", 6, 3, 1)]                    # c1: POS 2, REF A ALT ATT
    mixed = [(1, 4, 3, "GGC", 7, 5, 1),                        # c2: before byte 4 (A): anchor byte 3, POS 4, ALT TGGC
             (0, 14, 2, "AG", 0, 9, 2),                        # c1: AG after CAGAGAG: rotates to POS 8 (anchor C), ALT CAG
             (0, 7, 2, "TG", 6, 2, 1),                         # c1: before byte 7 (C): s[6] = T != G: stays, POS 7, ALT TTG
             (0, 7, 2, "GT", 6, 2, 1)]                         # c1: rotates through TTTTT to POS 2 (anchor A): ALT ATG -- LEN 2, before ATT
    txt = indels.vcf_text(31, 3, 4, names, [17, 10], seqs, recs, mixed)
    head = [ln for ln in txt.splitlines() if ln.startswith("#")]
    body = [ln for ln in txt.splitlines() if not ln.startswith("#")]
    assert head[1] == "##source=jasper_amd indel scan, k=31, threshold=3, max_len=4, mixed"
    assert [ln for ln in head if "ID=TYPE" in ln] == ['##INFO=<ID=TYPE,Number=1,Type=String,Description="ins: the reads hold LEN more bases; del: the reads lack LEN bytes">']
    assert body == ["c1\t2\t.\tA\tAT\t.\t.\tKIND=het;TYPE=ins;LEN=1;RC=6;AC=4",
                    "c1\t2\t.\tA\tATT\t.\t.\tKIND=het;TYPE=ins;LEN=2;RC=6;AC=3",
                    "c1\t2\t.\tAT\tA\t.\t.\tKIND=het;TYPE=del;LEN=1;RC=6;AC=5",
                    "c1\t6\t.\tT\tTTG\t.\t.\tKIND=het;TYPE=ins;LEN=2;RC=6;AC=2",
                    "c1\t7\t.\tT\tTTG\t.\t.\tKIND=het;TYPE=ins;LEN=2;RC=6;AC=2",
                    "c1\t8\t.\tC\tCAG\t.\t.\tKIND=error;TYPE=ins;LEN=2;RC=0;AC=9",
                    "c2\t4\t.\tT\tTGGC\t.\t.\tKIND=het;TYPE=ins;LEN=3;RC=7;AC=5"]
    # the same from a structured array in another order
    arr = np.zeros(len(mixed), dtype=MIXED_DTYPE)
    for i, (seq, pos, ln, y, rmin, amin, kind) in enumerate(reversed(mixed)):
        arr[i] = (pos, seq, rmin, amin, sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(y)), ln, kind, [0] * 5)
    assert indels.vcf_text(31, 3, 4, names, [17, 10], [s.encode() for s in seqs], recs, arr) == txt
    # an empty mixed list still marks the file; None leaves every byte what it was
    marked = indels.vcf_text(31, 3, 4, names, [17, 10], seqs, recs, [])
    old = indels.vcf_text(31, 3, 4, names, [17, 10], seqs, recs)
    assert old == indels.vcf_text(31, 3, 4, names, [17, 10], seqs, recs, None)
    assert "mixed" not in old and "copies of one base" in old
    assert [ln for ln in marked.splitlines() if not ln.startswith("#")] == [ln for ln in old.splitlines() if not ln.startswith("#")]
    assert marked.splitlines()[1].endswith(", mixed")


def test_record_tuples_decode_the_bases():
    from jasper_amd.table import MIXED_DTYPE, MixedInsertions
    arr = np.zeros(2, dtype=MIXED_DTYPE)
    arr[0] = (7, 0, 6, 2, 0b10_11_00_01, 4, 1, [0] * 5)        # C A T G: base 0 in the lowest pair
    arr[1] = (9, 1, 0, 3, 0xFFFFFFFF, 16, 2, [0] * 5)
    m = MixedInsertions([(1, 0, 0), (0, 1, 0)], arr, 0.0, 0, False)
    assert m.record_tuples() == [(0, 7, 4, "CATG", 6, 2, 1), (1, 9, 16, "T" * 16, 0, 3, 2)]


@pytest.mark.parametrize("module", ["jasper_amd.cli", "jasper_amd.kmerqc"])
def test_indel_mixed_needs_indels(module, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "r.fa"
    fq.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    args = ["-a", str(fa), "-r", str(fq), "-k", "5", "--indel-mixed"] + (["--threshold", "1"] if module.endswith("kmerqc") else [])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--indel-mixed needs --indels" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []
