"""GPU: the read-text path (KmerTable.read_bins_text, jasper_read_text_bins / jasper_read_text_fetch) against the line-by-line restatement
of its parser (tests/readtext_ref.py) for every field, and its counters against the restatement of the binning (tests/readbins_ref.py)
over the synthetic trio's parents.  Nothing expected here comes from the code under test; that the restatement equals the host parser and
that the texts hold what they are meant to hold is tests/test_readtext_ref.py.

What the kernels can get wrong is where lines, records and blocks meet: a workgroup owns 4096 text bytes and a thread 16 of them, so the
texts put records across every block seam, one line over several blocks, line ends of every kind at the text's end, and more blocks
than one pass of the block-total scan takes (readtext_ref.SCAN_PASS_BLOCKS)."""
import ctypes as C

import numpy as np
import pytest

import readbins_ref as ref
import readtext_ref as rt

pytestmark = pytest.mark.gpu
K = rt.K
THRE = 2


class Trio:
    def __init__(self, KT):
        self.trio = t = ref.make_trio()
        self.md, self.pd = ref.kmer_dict([t["hap_a"]], K, 4), ref.kmer_dict([t["hap_b"]], K, 4)
        self.M, self.P = KT(K, min_slots=1 << 16), KT(K, min_slots=1 << 16)
        self.M.count_bases(b"N".join([t["hap_a"]] * 4))
        self.P.count_bases(b"N".join([t["hap_b"]] * 4))
        self.cases = {name: (fmt, text, eof) for name, fmt, text, eof in rt.cases(t)}
        self._counts = {}

    def counts(self, reads):
        """the restatement's counters, each distinct read counted once"""
        for r in set(reads) - set(self._counts):
            m, p = ref.read_counts([r], K, self.md, self.pd, THRE, THRE)
            self._counts[r] = (m[0], p[0])
        return [self._counts[r][0] for r in reads], [self._counts[r][1] for r in reads]


@pytest.fixture(scope="module")
def trio(hip):
    from jasper_amd import KmerTable
    t = Trio(KmerTable)
    yield t
    t.M.close()
    t.P.close()


def run(t, text, eof, fmt, want_seq=True):
    from jasper_amd import KmerTable
    return KmerTable.read_bins_text(t.M, t.P, text, eof, fmt, THRE, THRE, want_seq=want_seq)


def check(t, name, markers=None):
    fmt, text, eof = t.cases[name]
    used, rec_start, head_end, lens, seq = rt.parse(text, eof, fmt)
    reads = rt.reads_of(lens, seq)
    m, p = t.counts(reads)
    if markers is not None:                             # first, on the restatement alone: no vacuous input
        assert sum(1 for x, y in zip(m, p) if x + y) >= markers * len(reads), name
    r = run(t, text, eof, fmt)
    assert not r.malformed and (r.used, r.n_records) == (used, len(lens)), name
    assert r.rec_start.dtype == np.int64 and r.mat.dtype == np.uint32
    assert r.rec_start.tolist() == rec_start, name
    assert r.head_end.tolist() == head_end, name
    assert r.lens.tolist() == lens, name
    assert r.seq.tobytes() == seq, name
    assert r.mat.tolist() == m and r.pat.tolist() == p, name
    return r


def test_fastq_blocks_and_special_records(trio):
    """(a), (c): several blocks, records across every seam, the special records; at least 90 % of the reads carry a marker"""
    check(trio, "a", markers=0.9)
    check(trio, "a_not_eof")


@pytest.mark.parametrize("name", ["b_crlf", "b_no_last_lf", "b_last_cr_no_lf"])
def test_line_ends(trio, name):
    check(trio, name, markers=0.9)


def test_cut_chunks(trio):
    """(d): the chunk ends inside each line of its last record, or right behind a record: used is the last whole record's end"""
    names = [n for n in trio.cases if n.startswith("d_")]
    assert len(names) == 5
    useds = {check(trio, n).used for n in names}
    assert len(useds) == 1


def test_one_long_read(trio):
    """(e): one line over several blocks"""
    r = check(trio, "e_long_read")
    assert r.lens.tolist()[1] == 3 * rt.BLOCK + 5 and r.mat[1] + r.pat[1] > 0


@pytest.mark.parametrize("name", ["f_fasta", "f_fasta_not_eof", "f_fasta_crlf", "f_fasta_no_last_lf", "f_fasta_cut"])
def test_fasta(trio, name):
    check(trio, name, markers=0.9)


def test_malformed(trio):
    """(g): one text per verdict of the host parser; the first bad record is the restatement's and lies beyond the first block"""
    for name, text, eof, what in rt.malformed(trio.trio):
        with pytest.raises(rt.Bad) as e:
            rt.parse(text, eof, "fastq")
        assert e.value.what == what
        r = run(trio, text, eof, "fastq")
        assert r.malformed and r.bad_record == e.value.record, name
        assert r.mat is None and r.rec_start is None
        if what == rt.ENDS_INSIDE:
            assert r.bad_record == r.n_records
    check(trio, "a")                                    # and the tables and the workspace are as good as before


def test_long_text(trio):
    """(h): more blocks than one pass of the block-total scan takes (SCAN_PASS_BLOCKS)"""
    fmt, text, eof = trio.cases["h_long_text"]
    assert len(text) > rt.SCAN_PASS_BLOCKS * rt.BLOCK
    check(trio, "h_long_text", markers=0.9)


def test_refusals(trio):
    """(i): every refusal is a host check"""
    from jasper_amd import KmerTable, _lib
    L = _lib.lib()
    used, n, bad, status = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
    some = b"@r\nACGT\n+\nIIII\n"

    def call(length):
        return L.jasper_read_text_bins(trio.M._h, trio.P._h, C.c_char_p(some), length, 1, 0, THRE, THRE, C.byref(used), C.byref(n), C.byref(status), C.byref(bad), None)

    for length in (1 << 31, (1 << 31) + 5, 1 << 40):    # a length, not a buffer: refused before the text is looked at
        assert call(length) != 0
        assert "2^31" in L.jasper_last_error().decode()
    assert call(-1) != 0
    r = check(trio, "a")
    rec = np.zeros(r.n_records + 2, dtype=np.int64)
    cnt = np.zeros(r.n_records + 1, dtype=np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)             # noqa: E731
    for wrong in (r.n_records - 1, r.n_records + 1, 0):
        assert L.jasper_read_text_fetch(trio.M._h, wrong, p(rec), p(rec), p(rec), p(cnt), p(cnt), None) != 0
        assert "n_records" in L.jasper_last_error().decode()
    assert L.jasper_read_text_fetch(trio.M._h, r.n_records, p(rec), p(rec.copy()), p(rec.copy()), p(cnt), p(cnt.copy()), None) == 0
    assert rec[:r.n_records + 1].tolist() == r.rec_start.tolist()
    # a binning call of the other kind spoils what could be fetched; a malformed chunk leaves nothing
    KmerTable.read_bins(trio.M, trio.P, [b"ACGT" * 20], THRE, THRE)
    assert L.jasper_read_text_fetch(trio.M._h, r.n_records, p(rec), p(rec), p(rec), p(cnt), p(cnt), None) != 0
    with pytest.raises(Exception, match="the same table"):            # (check_trio's refusals, as read_bins has them)
        KmerTable.read_bins_text(trio.M, trio.M, some, True, "fastq", THRE, THRE)
    with pytest.raises(Exception, match="maternal threshold must be at least 1"):
        KmerTable.read_bins_text(trio.M, trio.P, some, True, "fastq", 0, THRE)
    with pytest.raises(ValueError):
        KmerTable.read_bins_text(trio.M, trio.P, some, True, "sam", THRE, THRE)
    empty = run(trio, b"", True, "fastq")
    assert (empty.used, empty.n_records, empty.malformed) == (0, 0, False) and empty.rec_start.tolist() == [0]
    partial = run(trio, b"@r\nACGT\n+\nII", False, "fastq")
    assert (partial.used, partial.n_records, partial.malformed) == (0, 0, False)
    one_header = run(trio, b">r\nACGT\n", False, "fasta")
    assert (one_header.used, one_header.n_records) == (0, 0)
    check(trio, "a")
