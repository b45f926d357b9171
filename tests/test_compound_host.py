"""CPU: the compound scan.  The restatement of its semantics that the GPU tests compare against (test_gpu_compound.py,
test_gpu_cli_compound.py), checked here against a plain form by enumeration and on the committed dumps of the golden cases; and the
host side (jasper_amd/compound.py: the TSV, VCF and log texts; the flag errors of the driver and of kmerqc) on hand-made records.
Nothing expected here comes from the code under test.

Semantics (include/jasper_hip.h, jasper_compound_scan): s case folded; cnt = the count of a canonical k-mer, clamped to 2^32-1;
FRONT = 64; thre >= 1, k >= 2, 1 <= max_len <= 64.
  sites    a maximal run of unreliable windows (start, n_kmers, min_count) as the dense report lists it, R = n_kmers - k + 1:
           a site when 1 <= R <= max_len, long when R > max_len, neither when n_kmers < k.  a = start + k - 1, q = start + n_kmers,
           F = s[a-k+1 .. a-1], G = s[q .. q+k-2]; the contig's R bytes s[a .. q) are what is replaced.
  search   S_0 = {empty}; S_t = the one-base extensions yz of S_(t-1) with cnt(the last k bases of F + yz) >= thre.  It runs t = 1, 2, ..
           and ends at the first of: t > max_len, S_t empty, |S_t| > FRONT -- then the site is complex, counted once; the records of
           lengths < t stay and nothing of length >= t is listed.
  records  every y in a reached S_t whose windows t .. t+k-2 of F + y + G are >= thre too, except R = 1 and t = 1 (the variant
           scan's): (seq, pos = a, ref_len = R, len = t, y, ref_min = min_count, alt_min = the minimum over all k-1+t windows)
  ordered by (seq, pos, len, y); per sequence (sites, bridged, records, long, complex), bridged = sites with at least one record."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import Case, case_names
from test_gpu_copies import as_bytes, dict_counter, kmer_dict
from test_gpu_kmer_report import restate as restate_runs
from test_gpu_kmer_report import window_counts
from test_indels_host import ACGT, U32, rand_bases

FRONT = 64


def _finish(recs, per_seq):
    recs.sort(key=lambda r: (r[0], r[1], r[3], r[4]))
    counts = []
    for si, (sites, long_, complex_) in enumerate(per_seq):
        mine = [r for r in recs if r[0] == si]
        counts.append((sites, len({r[1] for r in mine}), len(mine), long_, complex_))
    return counts, recs


def restate_compound(seqs, k, count, thre, max_len, stats=None):
    """(counts, records) of the semantics above; count(bytes of k upper-case bases) -> int.  Shortcuts: the runs are those of the
    report's restatement (test_gpu_kmer_report.restate), the frontier is carried from level to level with its running minimum, and
    the rejoin windows stop at the first one below thre.  stats, a dict, gets `sites`, `long`, `complex`, `widest` (the largest level
    that was searched), `levels` (the sizes of all levels that were computed, those above FRONT too) and `longest` (the longest y)."""
    recs, per_seq = [], []
    st = dict(sites=0, long=0, complex=0, widest=0, levels=[], longest=0)
    for si, s in enumerate(seqs):
        up = as_bytes(s).upper()
        sites = long_ = complex_ = 0
        for _, start, nk, _, rmin in restate_runs([window_counts(s, k, count)], thre)[1]:
            R = nk - k + 1
            if R < 1:
                continue
            if R > max_len:
                long_ += 1
                continue
            sites += 1
            a, q = start + k - 1, start + nk
            F, G = up[a - k + 1:a], up[q:q + k - 1]
            assert len(F) == k - 1 and len(G) == k - 1 and all(ch in ACGT for ch in F + G)
            S = [(b"", U32)]
            for t in range(1, max_len + 1):
                new = []
                for y, m in S:
                    for z in ACGT:
                        c = min(count((F + y + bytes([z]))[-k:]), U32)
                        if c >= thre:
                            new.append((y + bytes([z]), min(m, c)))
                st["levels"].append(len(new))
                if len(new) > FRONT:
                    complex_ += 1
                    break
                if not new:
                    break
                S = new
                st["widest"] = max(st["widest"], len(S))
                if R == 1 and t == 1:
                    continue
                for y, m in S:
                    alt = (F + y + G)[t:]                             # windows t .. t+k-2
                    amin = m
                    for j in range(k - 1):
                        amin = min(amin, min(count(alt[j:j + k]), U32))
                        if amin < thre:
                            break
                    if amin >= thre:
                        recs.append((si, a, R, t, y.decode(), rmin, amin))
                        st["longest"] = max(st["longest"], t)
        per_seq.append((sites, long_, complex_))
        st["sites"] += sites
        st["long"] += long_
        st["complex"] += complex_
    if stats is not None:
        stats.update(st)
    return _finish(recs, per_seq)


def restate_compound_plain(seqs, k, count, thre, max_len):
    """the same straight from the definition: the runs from a loop over the windows, every string y of every length, every minimum over
    all its windows; the level sizes |S_t| computed separately, as the number of strings of length t all of whose t windows of F + y
    are solid"""
    recs, per_seq = [], []
    for si, s in enumerate(seqs):
        b = as_bytes(s)
        up, n = b.upper(), len(b)

        def cmin(x):
            return min(min(count(x[j:j + k]), U32) for j in range(len(x) - k + 1))

        unrel = [all(ch in b"ACGTacgt" for ch in b[i:i + k]) and min(count(up[i:i + k]), U32) < thre for i in range(max(0, n - k + 1))]
        sites = long_ = complex_ = 0
        i = 0
        while i < len(unrel):
            if not unrel[i]:
                i += 1
                continue
            j = i
            while j < len(unrel) and unrel[j]:
                j += 1
            start, nk = i, j - i
            i = j
            R = nk - k + 1
            if R < 1:
                continue
            if R > max_len:
                long_ += 1
                continue
            sites += 1
            a, q = start + k - 1, start + nk
            F, G = up[a - k + 1:a], up[q:q + k - 1]
            rmin = cmin(up[start:start + nk + k - 1])
            reached = 0                                               # the levels 1 .. reached are searched
            for t in range(1, max_len + 1):
                size = sum(1 for y in itertools.product(ACGT, repeat=t) if cmin(F + bytes(y)) >= thre)
                if size == 0:
                    break
                if size > FRONT:
                    complex_ += 1
                    break
                reached = t
            for t in range(1, reached + 1):
                if R == 1 and t == 1:
                    continue
                for y in itertools.product(ACGT, repeat=t):
                    amin = cmin(F + bytes(y) + G)
                    if amin >= thre:
                        recs.append((si, a, R, t, bytes(y).decode(), rmin, amin))
        per_seq.append((sites, long_, complex_))
    return _finish(recs, per_seq)


def substitute(s, at):
    """s with the bytes at the given positions replaced by the next base (A -> C -> G -> T -> A)"""
    b = bytearray(s)
    for p in at:
        b[p] = ACGT[(ACGT.index(b[p]) + 1) & 3]
    return bytes(b)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def tiny_fuzz(k, seed=412):
    """reads that hold g twice and a second haplotype twice; contigs made of g with clustered errors, an N, lower case, short ones"""
    rng = np.random.default_rng(seed + k)
    g = rand_bases(rng, 160)
    g2 = substitute(g, [40, 100])
    c1 = bytearray(substitute(g, [20, 22, 50, 50 + k - 1, 90, 91]))
    del c1[120:122]                                               # a length error next to a substitution
    c1 = bytes(substitute(bytes(c1), [117]))
    c2 = bytearray(substitute(g, [2, 4, 70, 72, 155, 157]))       # runs that start at window 0 and end at the last one
    c2[60] = ord("N")
    c2[66:80] = bytes(c2[66:80]).lower()
    c3 = substitute(g, [30, 30 + k])                              # k apart: R = k + 1
    return [g] * 2 + [g2] * 2, [c1, bytes(c2), c3, g[:k - 1], b"", g[10:10 + 2 * k]]


def test_the_restatement_agrees_with_its_plain_form():
    seen = dict(records=0, long=0, complex=0, sites=0)
    for k in (4, 5, 6):
        reads, seqs = tiny_fuzz(k)
        count = dict_counter(kmer_dict(reads, k))
        for thre, max_len in ((1, 1), (1, 5), (2, 3), (2, 5), (3, 4)):
            got = restate_compound(seqs, k, count, thre, max_len)
            assert got == restate_compound_plain(seqs, k, count, thre, max_len), (k, thre, max_len)
            for c in got[0]:
                seen["sites"] += c[0]
                seen["records"] += c[2]
                seen["long"] += c[3]
                seen["complex"] += c[4]
            assert all(c[1] <= c[0] and c[1] <= c[2] for c in got[0])
    assert seen["records"] > 20 and seen["long"] > 0 and seen["sites"] > 20, seen


def cap_workload():
    """(reads, contigs) at k = 4 and thre 1: one read of 90 random bases and a contig cut from it with two substitutions 2 apart, one
    site.  Its levels hold 1, 3, 11, 26, 64 and 155 prefixes: with max_len 5 the front just fits, from max_len 6 on the site is complex"""
    rng = np.random.default_rng(285)
    g = rand_bases(rng, 90)
    lo = int(rng.integers(10, 90 - 50))
    return [g], [substitute(g[lo:lo + 40], [18, 20])]


def test_a_level_wider_than_the_front_is_complex_once():
    reads, seqs = cap_workload()
    count = dict_counter(kmer_dict(reads, 4))
    st5, st6 = {}, {}
    want5 = restate_compound(seqs, 4, count, 1, 5, st5)
    want6 = restate_compound(seqs, 4, count, 1, 6, st6)
    assert st5["levels"] == [1, 3, 11, 26, FRONT] and st6["levels"] == [1, 3, 11, 26, FRONT, 155]
    assert want5[0] == [(1, 1, 41, 0, 0)] and want6[0] == [(1, 1, 41, 0, 1)]      # complex once, and the shorter records are kept
    assert want5[1] == want6[1] and {r[3] for r in want5[1]} == {2, 3, 4, 5}
    assert restate_compound(seqs, 4, count, 1, 64)[0] == want6[0]
    assert want5 == restate_compound_plain(seqs, 4, count, 1, 5) and want6 == restate_compound_plain(seqs, 4, count, 1, 6)


@pytest.mark.parametrize("k", [21, 31, 64])
def test_planted_pairs(k):
    """two substitutions d apart in a contig, reads = 5 copies of the truth: one record, y = the truth's bytes from the first to the
    second; at k = 64 and d = 64 the run is long; k + 3 apart they are two runs of k windows, which are the variant scan's"""
    truth, contig, pairs, far = planted_pairs(k)
    count = dict_counter(kmer_dict([truth] * 5, k))
    st = {}
    counts, recs = restate_compound([contig], k, count, 3, 64, st)
    want = [(0, p, d + 1, d + 1, truth[p:p + d + 1].decode(), 0, 5) for p, d in pairs if d + 1 <= 64]
    assert recs == want
    assert counts == [(len(want) + 2, len(want), len(want), 1 if k == 64 else 0, 0)]      # (the far pair: two sites with R = 1 and no record)
    assert st["widest"] == 1
    # the far pair gives two runs of exactly k windows: R = 1, the variant scan's
    runs = restate_runs([window_counts(contig, k, count)], 3)[1]
    assert [(r[1], r[2]) for r in runs if r[1] + k - 1 in far] == [(far[0] - k + 1, k), (far[1] - k + 1, k)]


def planted_pairs(k, seed=88):
    """(truth, contig, [(p, d)], (p1, p2)): pairs of substitutions at p and p + d for d in 1, 2, 3, 7, k-2, k-1 and k, one pair every
    4k bases, and one pair k + 3 apart"""
    rng = np.random.default_rng(seed + k)
    ds = (1, 2, 3, 7, k - 2, k - 1, k)
    truth = rand_bases(rng, 4 * k * (len(ds) + 2))
    at, pairs = [], []
    for i, d in enumerate(ds):
        p = 2 * k + 4 * k * i
        at += [p, p + d]
        pairs.append((p, d))
    p = 2 * k + 4 * k * len(ds)
    at += [p, p + k + 3]
    return truth, substitute(truth, at), pairs, (p, p + k + 3)


# ---- anchors on the committed dumps ----------------------------------------------------------------------------------------------
# (records, long runs, complex sites) at max_len 64; zeros in every other case
COMPOUND_ANCHORS = {"cluster_k25": (8, 0, 0), "cluster_k37": (9, 0, 0), "diploid_k25": (3, 0, 0), "gaps_k25": (5, 2, 0), "gaps_k37_p4": (4, 2, 0)}


@pytest.mark.parametrize("name", case_names())
def test_golden_anchors(name):
    c = Case(name)
    _, seqs = c.batch()
    count = dict_counter({key.encode(): v for key, v in c.dump().items()})
    st = {}
    counts, recs = restate_compound(seqs, c.k, count, c.thre, 64, st)
    assert (len(recs), st["long"], st["complex"]) == COMPOUND_ANCHORS.get(name, (0, 0, 0)), (name, recs)
    assert sum(x[2] for x in counts) == len(recs) and all(r[5] < c.thre <= r[6] for r in recs)


def test_the_anchors_name_golden_cases():
    assert set(COMPOUND_ANCHORS) <= set(case_names()) and len(case_names()) == 17


# ---- writers ---------------------------------------------------------------------------------------------------------------------
def test_tsv_and_log_texts():
    from jasper_amd import compound
    names = ["c1", "c2"]
    stages = [("before", [100, 50], [(4, 3, 5, 1, 1), (1, 0, 0, 2, 0)]), ("after", [99, 50], [(1, 1, 1, 0, 0), None])]      # c2: not in the polished FASTA
    assert compound.compound_tsv_text(names, stages) == (
        "#contig\tstage\tlength\tsites\tbridged\trecords\tlong\tcomplex\n"
        "c1\tbefore\t100\t4\t3\t5\t1\t1\nc1\tafter\t99\t1\t1\t1\t0\t0\n"
        "c2\tbefore\t50\t1\t0\t0\t2\t0\nc2\tafter\t0\t0\t0\t0\t0\t0\n"
        "*\tbefore\t150\t5\t3\t5\t3\t1\n*\tafter\t99\t1\t1\t1\t0\t0\n")
    assert compound.compound_tsv_text(["c"], [("asm", [7], [(0, 0, 0, 0, 0)])]) == (
        "#contig\tstage\tlength\tsites\tbridged\trecords\tlong\tcomplex\nc\tasm\t7\t0\t0\t0\t0\t0\n*\tasm\t7\t0\t0\t0\t0\t0\n")
    assert compound.stage_log_text(stages[0][2]) == "5 sites, 3 bridged, 5 records, 3 long runs, 1 complex sites"
    assert compound.log_text(stages[0][2], stages[1][2]) == ("Compound scan: before polishing 5 sites, 3 bridged, 5 records, 3 long runs, 1 complex sites; "
                                                             "after polishing 1 sites, 1 bridged, 1 records, 0 long runs, 0 complex sites")


def test_vcf_text():
    from jasper_amd import compound
    from jasper_amd.table import COMPOUND_DTYPE, CompoundScan, KmerReport
    long_y = "ACGT" * 16
    names, seqs = ["c1", "c2"], ["GATTacaTCAGAGAGCTN", "ACGTACGTAC" * 8]
    recs = [(1, 3, 64, 64, long_y[1:] + "A", 1, 4),            # c2: len 64, as long as what it replaces
            (0, 4, 3, 3, "GCT", 0, 7),                         # c1: POS 5, REF aca as it stands in the file, an MNP
            (0, 4, 3, 2, "GT", 0, 9),                          # c1: the same site, shorter than REF: complex, before the MNP (LEN)
            (0, 4, 3, 3, "CCT", 0, 6),                         # c1: the same site and length: ALT order
            (0, 9, 2, 5, "TTGCA", 2, 3)]                       # c1: longer than REF: complex
    txt = compound.vcf_text(31, 3, 64, names, [18, 80], seqs, recs)
    head = [ln for ln in txt.splitlines() if ln.startswith("#")]
    body = [ln for ln in txt.splitlines() if not ln.startswith("#")]
    assert head[:4] == ["##fileformat=VCFv4.2", "##source=jasper_amd compound scan, k=31, threshold=3, max_len=64", "##contig=<ID=c1,length=18>",
                        "##contig=<ID=c2,length=80>"]
    assert [ln.split(",")[0] for ln in head[4:-1]] == ["##INFO=<ID=%s" % x for x in ("KIND", "TYPE", "RLEN", "LEN", "RC", "AC")]
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    assert body == ["c1\t5\t.\taca\tGT\t.\t.\tKIND=error;TYPE=complex;RLEN=3;LEN=2;RC=0;AC=9",
                    "c1\t5\t.\taca\tCCT\t.\t.\tKIND=error;TYPE=mnp;RLEN=3;LEN=3;RC=0;AC=6",
                    "c1\t5\t.\taca\tGCT\t.\t.\tKIND=error;TYPE=mnp;RLEN=3;LEN=3;RC=0;AC=7",
                    "c1\t10\t.\tAG\tTTGCA\t.\t.\tKIND=error;TYPE=complex;RLEN=2;LEN=5;RC=2;AC=3",
                    "c2\t4\t.\t%s\t%s\t.\t.\tKIND=error;TYPE=mnp;RLEN=64;LEN=64;RC=1;AC=4" % (seqs[1][3:67], long_y[1:] + "A")]
    # the same from a structured array in another order and from sequences as bytes; record_tuples gives the tuples back
    arr = np.zeros(len(recs), dtype=COMPOUND_DTYPE)
    for i, (seq, pos, rlen, ln, y, rmin, amin) in enumerate(reversed(recs)):
        v = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(y))
        arr[i] = (pos, seq, rmin, amin, rlen, [v & (2**64 - 1), v >> 64], ln, [0] * 6)
    assert compound.vcf_text(31, 3, 64, names, [18, 80], [s.encode() for s in seqs], arr) == txt
    cs = CompoundScan([], arr, KmerReport([], np.zeros(0), 0.0, False), 0.0, 0.0, 0, False)
    assert cs.record_tuples() == list(reversed(recs))
    # no record: the header alone
    assert [ln for ln in compound.vcf_text(31, 3, 64, names, [18, 80], seqs, []).splitlines() if not ln.startswith("#")] == []


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def _run(module, args, cwd):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("module", ["jasper_amd.cli", "jasper_amd.kmerqc"])
@pytest.mark.parametrize("bad", ["0", "65", "-1", "x", "6.5"])
def test_a_bad_length_ends_the_run(module, bad, tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "r.fa"
    fq.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    args = ["-a", str(fa), "-r", str(fq), "-k", "5", "--compound", "--compound-max-len", bad] + (["--threshold", "1"] if module.endswith("kmerqc") else [])
    r = _run(module, args, tmp_path)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "--compound-max-len takes an integer from 1 to 64; it is %s" % bad in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name not in ("a.fa", "r.fa")] == []


def test_threshold_zero_ends_kmerqc(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    r = _run("jasper_amd.kmerqc", ["-a", str(fa), "-r", str(fa), "-k", "5", "--compound", "--threshold", "0"], tmp_path)
    assert r.returncode == 1 and "--compound needs a threshold of at least 1; --threshold 0 was given" in r.stdout + r.stderr
    assert [f.name for f in tmp_path.iterdir() if f.name != "a.fa"] == []


def test_threshold_zero_ends_the_driver(capsys):
    """the driver takes its threshold from threshold.txt after the polishing: its scan function refuses 0 before it touches the table"""
    from jasper_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.scan_compound(None, [(">c", "ACGT")], 0, 64)
    assert e.value.code == 1
    out = capsys.readouterr()
    assert "--compound needs a threshold for unreliable kmers of at least 1; it is 0" in out.out + out.err
    assert cli.compound_flags(None) == 64 and cli.compound_flags("1") == 1 and cli.compound_flags("64") == 64
