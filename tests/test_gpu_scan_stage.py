"""GPU: what the five dense scans (k-mer report, copy-number scan, variant scan, indel scan, hap-mer scan) do with their INPUT, through the
host-text and the device-text entry point of each: offsets that decrease, nothing to scan, and one input given to all five in a row on the
same tables.  What the scans compute is the business of test_gpu_kmer_report.py, test_gpu_copies.py, test_gpu_variants.py,
test_gpu_indels.py and test_gpu_hapmers.py; here a result is compared with the empty result, or with the same scan's result from tables
nothing else has used."""
import numpy as np
import pytest
import torch

from test_gpu_copies import TILE

pytestmark = pytest.mark.gpu

K, THRE, PEAK = 21, 2, 3
SCANS = ("kmer report", "copy report", "variant scan", "indel scan", "hap-mer scan")      # (the prefix of each scan's error messages)
EMPTY_COUNTS = {"kmer report": (0, 0, 0, 0), "copy report": (0,) * 6, "variant scan": (0, 0, 0), "indel scan": (0, 0, 0, 0), "hap-mer scan": (0, 0, 0, 0)}
RUN_SCANS = ("kmer report", "copy report", "hap-mer scan")      # (their lists are .runs, the others' .records)


def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def workload():
    """a few hundred bases of reads -- a 300-base piece 3 times, twice more with one base replaced and twice more with one base taken out --
    and three sequences of k - 1, k and TILE + k bases (0, 1 and TILE + 1 windows: the last one's second tile holds exactly one window).
    The long one holds the piece in its middle, so its last windows are an unreliable run across the tile seam."""
    rng = np.random.default_rng(12)
    g = rand_bases(rng, 300)
    sub = g[:150] + (b"A" if g[150:151] != b"A" else b"C") + g[151:]
    dele = g[:80] + g[81:]
    reads = b"N".join([g] * 3 + [sub] * 2 + [dele] * 2)
    long_ = bytearray(rand_bases(rng, TILE + K))
    long_[1000:1300] = g
    return reads, [rand_bases(rng, K - 1), g[:K], bytes(long_)]


class Tables:
    """r: the reads (the hap-mer scan's child), a: the sequences themselves, m and p: the hap-mer scan's mother and father, the first and
    the last third of the reads' text (m has the piece whole, p only with one base taken out: the windows over that base are maternal)"""

    def __init__(self, KT, reads, seqs):
        third = len(reads) // 3
        self.r, self.a, self.m, self.p = (KT(K, min_slots=1 << 16) for _ in range(4))
        self.r.count_bases(reads)
        self.a.count_bases(b"N".join(seqs))
        self.m.count_bases(reads[:third])
        self.p.count_bases(reads[-third:])

    def close(self):
        for t in (self.r, self.a, self.m, self.p):
            t.close()

    def host(self, scan, seqs):
        r = self.r
        return {"kmer report": lambda: r.kmer_report(seqs, THRE), "copy report": lambda: r.copy_report(self.a, seqs, THRE, PEAK),
                "variant scan": lambda: r.variant_scan(seqs, THRE), "indel scan": lambda: r.indel_scan(seqs, THRE, 4),
                "hap-mer scan": lambda: r.hapmer_scan(self.m, self.p, seqs, 1, 1, 1)}[scan]()

    def device(self, scan, d_text, offs):
        r = self.r
        return {"kmer report": lambda: r.kmer_report_device(d_text, offs, THRE), "copy report": lambda: r.copy_report_device(self.a, d_text, offs, THRE, PEAK),
                "variant scan": lambda: r.variant_scan_device(d_text, offs, THRE), "indel scan": lambda: r.indel_scan_device(d_text, offs, THRE, 4),
                "hap-mer scan": lambda: r.hapmer_scan_device(self.m, self.p, d_text, offs, 1, 1, 1)}[scan]()


def on_device(seqs):
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    d = torch.frombuffer(bytearray(b"".join(seqs) + bytes(16)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return d, offs


@pytest.fixture(scope="module")
def W(hip):
    from jasper_amd import KmerTable
    assert KmerTable.report_tile_windows() == TILE
    reads, seqs = workload()
    return KmerTable, reads, seqs


@pytest.fixture(scope="module")
def tables(W):
    t = Tables(*W)
    yield t
    t.close()


@pytest.mark.parametrize("scan", SCANS)
def test_decreasing_offsets_are_that_scans_error(tables, scan):
    from jasper_amd import _lib
    d, _ = on_device([b"ACGT" * 20])
    for offs in ([10, 5], [0, 40, 30, 80]):
        with pytest.raises(_lib.JasperHipError) as e:
            tables.device(scan, d, offs)
        assert str(e.value).startswith("libjasper_hip: " + scan + ": "), str(e.value)
    import ctypes as C
    L, res = _lib.lib(), C.c_void_p()
    cs, lens = (C.c_char_p * 2)(b"ACGT" * 20, b"ACGT"), (C.c_int64 * 2)(80, -1)      # the host text's counterpart: a negative length
    rc = {"kmer report": lambda: L.jasper_kmer_report(tables.r._h, 2, cs, lens, THRE, C.byref(res)),
          "copy report": lambda: L.jasper_copy_report(tables.r._h, tables.a._h, 2, cs, lens, THRE, PEAK, C.byref(res)),
          "variant scan": lambda: L.jasper_variant_scan(tables.r._h, 2, cs, lens, THRE, C.byref(res)),
          "indel scan": lambda: L.jasper_indel_scan(tables.r._h, 2, cs, lens, THRE, 4, C.byref(res)),
          "hap-mer scan": lambda: L.jasper_hapmer_scan(tables.m._h, tables.p._h, tables.r._h, 2, cs, lens, 1, 1, 1, C.byref(res))}[scan]()
    assert rc != 0 and not res
    assert L.jasper_last_error().decode().startswith(scan + ": "), L.jasper_last_error()


def check_empty(scan, res, n):
    assert res.counts == [EMPTY_COUNTS[scan]] * n, (scan, res.counts)      # (the report's first counter is the sequence's windows: 0 below k bases)
    assert not res.retried, scan
    assert len(res.runs if scan in RUN_SCANS else res.records) == 0, scan
    if scan == "variant scan":
        assert res.candidates == 0
    if scan == "indel scan":
        check_empty("variant scan", res.variants, n)
        assert res.lookups == 0


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("seqs", [[], [b""], [b"ACGTACGTAC", b"", b"A" * (K - 1)]], ids=["no_sequence", "one_empty", "all_below_k"])
def test_nothing_to_scan_gives_an_empty_result(tables, scan, seqs):
    check_empty(scan, tables.host(scan, seqs), len(seqs))
    d, offs = on_device(seqs)
    check_empty(scan, tables.device(scan, d, offs), len(seqs))


def test_scans_in_a_row_equal_each_scan_on_fresh_tables(W, tables):
    KT, reads, seqs = W
    assert [len(s) for s in seqs] == [K - 1, K, TILE + K]
    d, offs = on_device(seqs)
    got = [tables.host(scan, seqs) for scan in SCANS] + [tables.device(scan, d, offs) for scan in SCANS]
    for i, scan in enumerate(SCANS * 2):
        fresh = Tables(KT, reads, seqs)
        want = fresh.host(scan, seqs)
        fresh.close()
        assert got[i] == want, (scan, "host text" if i < len(SCANS) else "device text")
        assert not got[i].retried
    rep, cop, var, ind, hap = got[:len(SCANS)]
    assert [c[0] for c in rep.counts] == [0, 1, TILE + 1]
    assert [c[0] for c in cop.counts] == [0, 1, TILE + 1]
    runs = rep.run_tuples()
    assert runs and runs[-1][0] == 2 and runs[-1][1] + runs[-1][2] == TILE + 1      # the last run ends with the one window of the second tile
    assert len(cop.runs) > 0 and len(var.records) > 0 and ind.variants == var
    assert [c[0] for c in hap.counts] == [0, 1, TILE + 1]
    assert (2, 1000 + 80 - (K - 1), K, 1) in hap.run_tuples()      # the K windows over the base that the father's reads lack, in the piece at 1000
