"""CPU: the line-by-line restatement of the read-text parser (tests/readtext_ref.py) held equal to the host parser of the trio tool
(jasper_amd.triobin: _fastq_chunk / _fasta_chunk) on every crafted text the GPU test runs on -- and the texts are shown to hold what they
are meant to hold, so that neither test passes on a vacuous input."""
import numpy as np
import pytest

import readbins_ref as ref
import readtext_ref as rt
from jasper_amd import triobin


@pytest.fixture(scope="module")
def trio():
    return ref.make_trio()


def host(text, eof, fmt):
    parse = triobin._fastq_chunk if fmt == "fastq" else triobin._fasta_chunk
    return parse(np.frombuffer(text, dtype=np.uint8), eof, "p", 0, True)


def test_restatement_equals_the_host_parser(trio):
    for name, fmt, text, eof in rt.cases(trio):
        used, rec_start, head_end, lens, seq = rt.parse(text, eof, fmt)
        h_used, ch = host(text, eof, fmt)
        assert used == h_used, name
        if ch is None:
            assert rec_start == [0] and not lens, name
            continue
        assert rec_start[:-1] == ch.rec_start.tolist() and rec_start[1:] == ch.rec_end.tolist(), name
        assert head_end == ch.head_end.tolist() and lens == ch.lens.tolist(), name
        assert seq == ch.seq.tobytes(), name
        assert len(lens) > 0, name


def test_malformed_verdicts_equal_the_host_parser(trio):
    seen = set()
    for name, text, eof, what in rt.malformed(trio):
        with pytest.raises(rt.Bad) as e:
            rt.parse(text, eof, "fastq")
        assert e.value.what == what, name
        with pytest.raises(triobin.Malformed) as h:
            host(text, eof, "fastq")
        assert str(h.value) == "p: record %d is malformed: %s" % (e.value.record, what), name
        # the bad record is not in the first block: the records before it, which the unspoilt text shares, cover more than a block
        good = rt.parse(b"".join(rt.base_records(trio)), True, "fastq")
        assert good[1][e.value.record] > rt.BLOCK, name
        seen.add(what)
    assert seen == {rt.NO_AT, rt.NO_PLUS, rt.UNEQUAL, rt.ENDS_INSIDE}


def test_texts_hold_what_they_are_meant_to(trio):
    by = {name: (fmt, text, eof) for name, fmt, text, eof in rt.cases(trio)}
    k = rt.K
    # (a): several blocks, a record across every block seam
    fmt, a, _ = by["a"]
    assert 20000 <= len(a) <= 30000
    _, starts, _, lens, seq = rt.parse(a, True, "fastq")
    seams = list(range(rt.BLOCK, len(a), rt.BLOCK))
    assert len(seams) >= 4 and not set(seams) & set(starts)
    # (c): the special records
    reads = rt.reads_of(lens, seq)
    assert 0 in lens and k - 1 in lens and k in lens
    recs = rt.base_records(trio)
    quals = [r.split(b"\n")[3] for r in recs]
    assert any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
    assert any(b"\r" in r for r in reads) and any(r != r.upper() for r in reads) and any(b"N" in r for r in reads)
    assert b"\n\n+\n\n" in a                              # the empty read's empty quality line
    # (b)
    assert by["b_crlf"][1].count(b"\r\n") == by["b_crlf"][1].count(b"\n") == a.count(b"\n")
    assert not by["b_no_last_lf"][1].endswith(b"\n") and by["b_last_cr_no_lf"][1].endswith(b"I\r")
    for name in ("b_crlf", "b_no_last_lf", "b_last_cr_no_lf"):
        assert rt.parse(by[name][1], True, "fastq")[3:] == (lens, seq), name
    # (d): the cut falls inside each line of the last record and right behind the record before; used is that record's end every time
    want_used = starts[-2]
    cut_lines = set()
    for name in by:
        if name.startswith("d_"):
            text = by[name][1]
            assert by[name][2] is False and rt.parse(text, False, "fastq")[0] == want_used, name
            cut_lines.add(text[want_used:].count(b"\n") if len(text) > want_used else -1)
            assert len(text) == want_used or not text.endswith(b"\n"), name
    assert cut_lines == {-1, 0, 1, 2, 3}
    # (e): one line over several blocks
    _, _, _, elens, _ = rt.parse(by["e_long_read"][1], True, "fastq")
    assert elens == [150, 3 * rt.BLOCK + 5, 150]
    # (f)
    fa = by["f_fasta"][1]
    used, fstarts, _, flens, fseq = rt.parse(fa, True, "fasta")
    assert used == len(fa) and 0 in flens and b"\n\n" in fa and b">" in fseq
    bodies = [fa[s:e].split(b"\n")[1:-1] for s, e in zip(fstarts, fstarts[1:])]
    assert any(len(b) == 1 for b in bodies) and any(len(b) == 3 and len(set(map(len, b))) == 3 for b in bodies)
    nused, nstarts, _, nlens, _ = rt.parse(fa, False, "fasta")
    assert nused == fstarts[-2] and nlens == flens[:-1]
    assert rt.parse(by["f_fasta_crlf"][1], True, "fasta")[3:] == (flens, fseq) and b"\r\n\r\n" in by["f_fasta_crlf"][1]
    assert 0 < rt.parse(by["f_fasta_cut"][1], False, "fasta")[0] < len(by["f_fasta_cut"][1])
    # (h): more blocks than one pass of the block-total scan takes
    assert len(by["h_long_text"][1]) > rt.SCAN_PASS_BLOCKS * rt.BLOCK


def test_most_reads_carry_a_marker(trio):
    """what the GPU test asserts first, here on the restatement alone: a packing error cannot hide behind zero counters"""
    md, pd = ref.kmer_dict([trio["hap_a"]], rt.K, 4), ref.kmer_dict([trio["hap_b"]], rt.K, 4)
    for name in ("a", "f_fasta"):
        fmt, text, eof = {n: (f, t, e) for n, f, t, e in rt.cases(trio)}[name]
        _, _, _, lens, seq = rt.parse(text, eof, fmt)
        m, p = ref.read_counts(rt.reads_of(lens, seq), rt.K, md, pd, 2, 2)
        assert sum(1 for x, y in zip(m, p) if x + y) >= 0.9 * len(lens), name
