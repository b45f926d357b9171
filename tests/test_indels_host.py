"""CPU: the indel scan's host side (jasper_amd/indels.py: TSV, VCF, left alignment, log texts) on hand-made records, and the restatement
of the scan's semantics that the GPU tests compare against (test_gpu_indels.py, test_gpu_cli_indels.py), checked here against a plain
form without shortcuts and on a construction with planted events.  Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h, jasper_indel_scan): s of n bytes, case folded; F = s[p-k+1 .. p-1]; cnt = the count of a canonical k-mer,
clamped to 2^32-1.
  ins(p, x, L), 1 <= L <= max_len, x != s[p]: evaluated iff k-1 <= p <= n-k+1 and s[p-k+1 .. p+k-2] are all bases; alt_min = min of cnt
      over the k+L-1 windows of F + x^L + s[p .. p+k-2]; ref_min = min over the k-1 windows of s that start at p-k+1 .. p-1
  del(p, L), 1 <= L <= max_len, s[p+L] != s[p], x = s[p+L]: evaluated iff k-1 <= p, p+L+k-2 <= n-1 and s[p-k+1 .. p+L+k-2] are all
      bases; alt_min = min over the k-1 windows of F + s[p+L .. p+L+k-2]; ref_min = min over the k+L-1 windows of s that start at
      p-k+1 .. p+L-1
  a record (seq, p, type, L, x, ref_min, alt_min, kind) iff evaluated and alt_min >= thre; kind 1 (het) when ref_min >= thre, else 2;
  ordered by (seq, pos, ins before del, len, base); per sequence (ins_het, ins_error, del_het, del_error)."""
import numpy as np

from test_gpu_copies import as_bytes, dict_counter, kmer_dict

U32 = 2**32 - 1
HET, ERROR = 1, 2
ACGT = b"ACGT"
TYPE_NO = {"ins": 1, "del": 2}


def _windows_min(a, k, count, stop_below=0):
    m = U32
    for j in range(len(a) - k + 1):
        m = min(m, min(count(a[j:j + k]), U32))
        if m < stop_below:
            break
    return m


def _finish(recs, n_seqs):
    recs.sort(key=lambda r: (r[0], r[1], TYPE_NO[r[2]], r[3], r[4]))
    counts = [[0, 0, 0, 0] for _ in range(n_seqs)]
    for r in recs:
        counts[r[0]][2 * (TYPE_NO[r[2]] - 1) + r[7] - 1] += 1
    return [tuple(c) for c in counts], recs


def restate(seqs, k, count, thre, max_len):
    """(counts, records) of the semantics above; count(bytes of k upper-case bases) -> int.  Shortcuts: nothing is tried at (p, x)
    unless F + x is solid (it is window 0 of every alternative string there), an alternative is left at its first window below thre,
    and ref_min is computed only for the alternatives that passed"""
    recs = []
    for si, s in enumerate(seqs):
        b = as_bytes(s)
        n, up = len(b), as_bytes(s).upper()
        pre = [0] * (n + 1)
        for i, ch in enumerate(up):
            pre[i + 1] = pre[i] + (0 if ch in ACGT else 1)

        def bases(lo, hi):
            return 0 <= lo and hi <= n - 1 and pre[hi + 1] == pre[lo]

        for p in range(k - 1, n):
            if not bases(p - k + 1, p):
                continue
            F = up[p - k + 1:p]
            for x in ACGT:
                xb = bytes([x])
                if x == up[p] or min(count(F + xb), U32) < thre:
                    continue
                if bases(p - k + 1, p + k - 2):
                    for L in range(1, max_len + 1):
                        amin = _windows_min(F + xb * L + up[p:p + k - 1], k, count, thre)
                        if amin >= thre:
                            rmin = _windows_min(up[p - k + 1:p + k - 1], k, count)
                            recs.append((si, p, "ins", L, chr(x), rmin, amin, HET if rmin >= thre else ERROR))
                for L in range(1, max_len + 1):
                    if bases(p - k + 1, p + L + k - 2) and up[p + L] == x:
                        amin = _windows_min(F + up[p + L:p + L + k - 1], k, count, thre)
                        if amin >= thre:
                            rmin = _windows_min(up[p - k + 1:p + L + k - 1], k, count)
                            recs.append((si, p, "del", L, chr(x), rmin, amin, HET if rmin >= thre else ERROR))
    return _finish(recs, len(seqs))


def restate_plain(seqs, k, count, thre, max_len):
    """the same straight from the definitions: every p, x and L, every minimum over all its windows"""
    recs = []
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        n = len(up)

        def bases(lo, hi):
            return 0 <= lo and hi <= n - 1 and all(ch in ACGT for ch in up[lo:hi + 1])

        def cmin(a):
            return min(min(count(a[j:j + k]), U32) for j in range(len(a) - k + 1))

        for p in range(n):
            for L in range(1, max_len + 1):
                if k - 1 <= p <= n - k + 1 and bases(p - k + 1, p + k - 2):
                    for x in ACGT:
                        if x != up[p]:
                            amin = cmin(up[p - k + 1:p] + bytes([x]) * L + up[p:p + k - 1])
                            rmin = cmin(up[p - k + 1:p + k - 1])
                            if amin >= thre:
                                recs.append((si, p, "ins", L, chr(x), rmin, amin, HET if rmin >= thre else ERROR))
                if k - 1 <= p and p + L + k - 2 <= n - 1 and bases(p - k + 1, p + L + k - 2) and up[p + L] != up[p]:
                    amin = cmin(up[p - k + 1:p] + up[p + L:p + L + k - 1])
                    rmin = cmin(up[p - k + 1:p + L + k - 1])
                    if amin >= thre:
                        recs.append((si, p, "del", L, chr(up[p + L]), rmin, amin, HET if rmin >= thre else ERROR))
    return _finish(recs, len(seqs))


def rand_bases(rng, n):
    return np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def right_normalised_del(s, q, L):
    """the position at which the scan reports the deletion of s[q .. q+L-1]: moved right while the byte after equals the first"""
    while q + L < len(s) and s[q + L] == s[q]:
        q += 1
    return q


def plant(h, events):
    """h with events [(q, 'ins', L, x) | (q, 'del', L, None)] applied (positions in h, ascending) -> the other haplotype"""
    out, at = [], 0
    for q, typ, L, x in events:
        out.append(h[at:q])
        if typ == "ins":
            out.append(bytes([x]) * L)
            at = q
        else:
            at = q + L
    out.append(h[at:])
    return b"".join(out)


def planted_workload(seed=2024, n=6000):
    """a random haplotype, and a second one with 10 same-base insertions and 10 deletions of lengths 1..4, isolated (more than 150
    bytes apart); reads: 6 copies of the first, 5 of the second.  -> (h1, reads, expected records at thre <= 5 for any k <= 64)"""
    rng = np.random.default_rng(seed)
    h1 = rand_bases(rng, n)
    events, want = [], []
    for i in range(20):
        q = 200 + 280 * i + int(rng.integers(0, 40))
        L = 1 + i % 4
        if i % 2 == 0:
            x = ACGT[(ACGT.index(h1[q:q + 1]) + 1 + int(rng.integers(0, 3))) % 4]
            events.append((q, "ins", L, x))
            want.append((0, q, "ins", L, chr(x), 6, 5, HET))
        else:
            events.append((q, "del", L, None))
            p = right_normalised_del(h1, q, L)
            want.append((0, p, "del", L, chr(h1[p + L]), 6, 5, HET))
    h2 = plant(h1, events)
    assert len(h2) == n + sum(e[2] for e in events if e[1] == "ins") - sum(e[2] for e in events if e[1] == "del")
    return h1, [h1] * 6 + [h2] * 5, want


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def small_fuzz(k, seed=77):
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, 500)
    g2 = plant(g, [(60, "ins", 2, ord("A") if g[60] != ord("A") else ord("C")), (150, "del", 1, None), (300, "del", 3, None)])
    a = bytearray(g)
    a[200] = ord("N")
    a[400:420] = bytes(a[400:420]).lower()
    return [g] * 2 + [g2] * 2 + [g[100:300]], [bytes(a), g[:2 * k - 3], g[:2 * k - 2], g[10:10 + 2 * k - 1], b"", g[250:330] + b"x" + g[331:380]]


def test_the_restatement_agrees_with_its_plain_form():
    for k in (2, 3, 5):
        reads, seqs = small_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        for thre, max_len in ((1, 1), (2, 4), (3, 16)):
            got = restate(seqs, k, count, thre, max_len)
            assert got == restate_plain(seqs, k, count, thre, max_len), (k, thre, max_len)
            assert len(got[1]) > 50


def test_the_restatement_finds_exactly_the_planted_events():
    h1, reads, want = planted_workload()
    assert len(want) == 20 and sum(r[2] == "ins" for r in want) == 10
    for k in (21, 31):
        count = dict_counter(kmer_dict(reads, k))
        counts, recs = restate([h1], k, count, 3, 4)
        assert recs == sorted(want, key=lambda r: r[1]), k
        assert counts == [(10, 0, 10, 0)]
    # at a small k the result list is longer than the sequence
    counts, recs = restate([h1], 5, dict_counter(kmer_dict(reads, 5)), 3, 4)
    assert len(recs) > len(h1)


# ---- writers ---------------------------------------------------------------------------------------------------------------------
def test_left_align():
    from jasper_amd.indels import left_align
    #    0123456789012345
    s = "GATTTTTCAGAGAGCTN"
    assert left_align(s, 6, "del", 1, "C") == 2            # the deletion of one T of TTTTT, reported at its right end, moves to the run's start
    assert left_align(s, 5, 2, 2, "C") == 2 and left_align(s, 7, "del", 1, "A") == 7
    assert left_align(s, 7, "ins", 1, "T") == 2            # the insertion of a T after the run moves through it
    assert left_align(s, 7, "ins", 3, "T") == 2 and left_align(s, 7, 1, 1, "A") == 7
    assert left_align(s, 12, "del", 2, "C") == 8           # AG AG AG: the deletion of s[12..13] = AG moves through the dinucleotide repeat to CAGAGAG's C
    assert left_align("ACNTTTTG", 6, "del", 1, "G") == 3   # an N stops it: s[2] is no base
    assert left_align("ACnTTTTG".lower(), 6, "del", 1, "G") == 3
    assert left_align("TTTTTG", 4, "del", 1, "G") == 1 and left_align("TTTTTG", 5, "ins", 2, "T") == 1      # q = 1 stops it: the anchor is byte 0
    assert left_align("ttTTtG", 4, "del", 1, "G") == 1     # case folded
    assert left_align(b"GATTTTTCAG", 7, "ins", 1, ord("T")) == 2


def test_tsv_text():
    from jasper_amd import indels
    names = ["c1", "c2"]
    txt = indels.indels_tsv_text(names, [("before", [100, 50], [(1, 2, 3, 4), (0, 0, 1, 0)]), ("after", [99, 50], [(1, 0, 3, 0), None])])
    assert txt == ("#contig\tstage\tlength\tins_het\tins_error\tdel_het\tdel_error\n"
                   "c1\tbefore\t100\t1\t2\t3\t4\nc1\tafter\t99\t1\t0\t3\t0\n"
                   "c2\tbefore\t50\t0\t0\t1\t0\nc2\tafter\t0\t0\t0\t0\t0\n"
                   "*\tbefore\t150\t1\t2\t4\t4\n*\tafter\t99\t1\t0\t3\t0\n")
    assert indels.stage_log_text([(1, 2, 3, 4), (0, 0, 1, 0)]) == "1 het and 2 error insertions, 4 het and 4 error deletions"
    assert indels.log_text([(1, 2, 3, 4)], [(0, 0, 0, 1), None]) == ("Indel scan: before polishing 1 het and 2 error insertions, 3 het and 4 error deletions; "
                                                                    "after polishing 0 het and 0 error insertions, 0 het and 1 error deletions")


def test_vcf_text_and_the_order_of_its_lines():
    from jasper_amd import indels
    names, seqs = ["c1", "c2"], ["GATTTTTCAGAGAGCTN", "ACGTACGTAC"]
    recs = [(1, 4, "ins", 2, "G", 7, 5, 1),            # c2: GG before byte 4 (A): anchor byte 3, POS 4
            (0, 12, "del", 2, "C", 0, 9, 2),           # c1: AG of the repeat, left-aligned to POS 8, REF CAG ALT C
            (0, 6, "del", 1, "C", 6, 5, 1),            # c1: one T, left-aligned to POS 2, REF AT ALT A
            (0, 7, "ins", 1, "T", 6, 4, 1),            # c1: one more T: POS 2, REF A ALT AT -- before the deletion at the same POS
            (0, 7, "ins", 2, "T", 6, 3, 1),
            (0, 7, "ins", 1, "G", 2, 3, 2)]            # c1: a G before byte 7: POS 7, REF T ALT TG
    txt = indels.vcf_text(31, 3, 4, names, [17, 10], seqs, recs)
    head = [ln for ln in txt.splitlines() if ln.startswith("#")]
    body = [ln for ln in txt.splitlines() if not ln.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == "##source=jasper_amd indel scan, k=31, threshold=3, max_len=4"
    assert head[2:4] == ["##contig=<ID=c1,length=17>", "##contig=<ID=c2,length=10>"] and head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert sum(ln.startswith("##INFO=<ID=") for ln in head) == 5
    assert body == ["c1\t2\t.\tA\tAT\t.\t.\tKIND=het;TYPE=ins;LEN=1;RC=6;AC=4",
                    "c1\t2\t.\tA\tATT\t.\t.\tKIND=het;TYPE=ins;LEN=2;RC=6;AC=3",
                    "c1\t2\t.\tAT\tA\t.\t.\tKIND=het;TYPE=del;LEN=1;RC=6;AC=5",
                    "c1\t7\t.\tT\tTG\t.\t.\tKIND=error;TYPE=ins;LEN=1;RC=2;AC=3",
                    "c1\t8\t.\tCAG\tC\t.\t.\tKIND=error;TYPE=del;LEN=2;RC=0;AC=9",
                    "c2\t4\t.\tT\tTGG\t.\t.\tKIND=het;TYPE=ins;LEN=2;RC=7;AC=5"]
    # the same from a structured array in another order
    from jasper_amd.table import INDEL_DTYPE
    arr = np.zeros(len(recs), dtype=INDEL_DTYPE)
    for i, (seq, pos, typ, ln, base, rmin, amin, kind) in enumerate(reversed(recs)):
        arr[i] = (pos, seq, rmin, amin, ln, TYPE_NO[typ], ord(base), kind, [0] * 7)
    assert indels.vcf_text(31, 3, 4, names, [17, 10], [s.encode() for s in seqs], arr) == txt
    assert indels.vcf_text(31, 3, 4, names, [17, 10], seqs, []).splitlines() == head
