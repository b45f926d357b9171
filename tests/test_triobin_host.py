"""CPU: the host side of `python -m jasper_amd.triobin` -- the reader, the rule, the writer, the flag checks -- and the restatement the GPU
tests compare with (tests/readbins_ref.py), on examples worked by hand.  The counting itself is replaced here by the restatement: the
tool's bin_files takes the counter as an argument, and the GPU tests (test_gpu_read_bins.py, test_gpu_cli_triobin.py) put the kernel there."""
import gzip
import os

import numpy as np
import pytest

import readbins_ref as ref

K = 5
MARK = b"AACCG"                       # canonical: its reverse complement is CGGTT


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------------
def counts(reads, md, pd, tm=1, tp=1, k=K):
    return ref.read_counts(reads, k, md, pd, tm, tp)


def test_restatement_on_examples_worked_by_hand():
    assert ref.canonical(MARK) == MARK and ref.canonical(b"CGGTT") == MARK
    md, pd = {MARK: 2}, {b"AAAAC": 3}
    # a marker inside a read counts once; the windows around it are no markers
    assert counts([b"TTAACCGTT"], md, pd) == ([1], [0])
    # the same k-mer split across two adjacent reads counts nowhere, at every cut
    for cut in range(3, 3 + K - 1):
        assert counts([b"TTAACCGTT"[:cut], b"TTAACCGTT"[cut:]], md, pd) == ([0, 0], [0, 0]), cut
    # ... and packed text with offsets is the same thing
    text, offs = ref.pack([b"TTAAC", b"CGTT", b"", b"AACCG"])
    assert offs == [0, 5, 9, 9, 14] and counts(ref.split(text, offs), md, pd) == ([0, 0, 0, 1], [0, 0, 0, 0])
    # reverse complement, lower case
    assert counts([b"TTCGGTTAA", b"ttaaCCgtt"], md, pd) == ([1, 1], [0, 0])
    # N (any non-base byte) inside the window: no k-mer; beside it: counted
    assert counts([b"TTAACNCGTT", b"TTAACCGNT", b"AAC-CG"], md, pd) == ([0, 1, 0], [0, 0, 0])
    # the father's k-mer, twice in one read (AAAAC and its reverse complement GTTTT)
    assert counts([b"AAAACGTTTT"], md, pd) == ([0], [2])
    # thresholds: a count below the threshold is no marker; a single occurrence in the other parent kills it
    assert counts([b"TTAACCGTT"], md, pd, tm=2) == ([1], [0]) and counts([b"TTAACCGTT"], md, pd, tm=3) == ([0], [0])
    assert counts([b"TTAACCGTT"], md, {MARK: 1}) == ([0], [0])
    assert counts([b"TTAACCGTT"], {MARK: 2**40}, pd, tm=ref.U32) == ([1], [0])      # clamped to 2^32-1, which still qualifies
    # shorter than k, empty
    assert counts([b"AACC", b""], md, pd) == ([0, 0], [0, 0])
    assert ref.hapmer_total(md, pd, 1) == 1 and ref.hapmer_total(md, pd, 3) == 0 and ref.hapmer_total(md, {MARK: 1}, 1) == 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
RULE_CASES = [
    # m, p, M_total, P_total, min_markers, bin
    (0, 0, 10, 10, 1, "unknown"),
    (1, 0, 10, 10, 1, "mat"),
    (0, 1, 10, 10, 1, "pat"),
    (2, 2, 10, 10, 1, "unknown"),                       # a tie
    (2, 4, 10, 20, 1, "unknown"),                       # a tie by the totals: 2 * 20 == 4 * 10
    (2, 3, 10, 20, 1, "mat"),                           # fewer maternal windows, but the mother has half as many markers
    (1, 0, 10, 10, 2, "unknown"),                       # --min-markers
    (1, 1, 10, 11, 2, "mat"),
    (3, 0, 10, 10, 3, "mat"),
    (2**32 - 1, 2**32 - 1, 2**40, 2**40 - 1, 1, "pat"),      # products of 2^72
    (2**32 - 1, 2**32 - 2, 2**40, 2**40, 1, "mat"),
    (2**24, 1, 5, 2**40, 1, "mat"),                     # m * P_total = 2^64: 0 in 64-bit arithmetic, which would say pat
    (1, 2**24, 2**40, 5, 1, "pat"),
]


def test_rule_is_exact_integer_arithmetic():
    from jasper_amd import triobin
    for m, p, mt, pt, mm, want in RULE_CASES:
        assert ref.bin_of(m, p, mt, pt, mm) == want, (m, p, mt, pt, mm)
        got = triobin.bin_codes(np.array([m, 0], dtype=np.uint64), np.array([p, 0], dtype=np.uint64), mt, pt, mm)
        assert [triobin.BINS[c] for c in got] == [want, "unknown"], (m, p, mt, pt, mm)
    # all cases of one pair of totals at once, the wide ones too
    for mt, pt in ((10, 20), (2**40, 2**40 - 1)):
        ms = [c[0] for c in RULE_CASES]
        ps = [c[1] for c in RULE_CASES]
        got = triobin.bin_codes(np.array(ms, dtype=np.uint64), np.array(ps, dtype=np.uint64), mt, pt, 1)
        assert [triobin.BINS[c] for c in got] == [ref.bin_of(m, p, mt, pt, 1) for m, p in zip(ms, ps)]
    assert len(triobin.bin_codes(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 3, 4, 1)) == 0


def test_pairs_are_decided_by_their_sums():
    ms, ps = [[3, 0, 1, 0], [0, 0, 1, 0]], [[0, 1, 0, 0], [2, 4, 1, 0]]
    assert ref.file_bins(ms, ps, 10, 10) == [["mat", "pat", "mat", "unknown"], ["pat", "pat", "unknown", "unknown"]]
    # sums (3, 2), (0, 5), (2, 1), (0, 0): both mates get their template's bin
    assert ref.file_bins(ms, ps, 10, 10, paired=True) == [["mat", "pat", "mat", "unknown"]] * 2
    assert ref.file_bins(ms, ps, 10, 10, min_markers=4, paired=True) == [["mat", "pat", "unknown", "unknown"]] * 2


# ---- the reader and the writer ------------------------------------------------------------------------------------------------------
READS = [("r0", b"TTAACCGTT"), ("r1 extra words", b"AAAACGTTTT"), ("r2", b""), ("r3", b"ttaaccgttNAAAAC"), ("r4", b"AACC"), ("r5", b"GGGGGGGGGGGG")]
MD, PD = {MARK: 2}, {b"AAAAC": 3}
M_TOTAL, P_TOTAL = 7, 5


def fasta_text(reads, width=None, eol=b"\n"):
    out = b""
    for name, s in reads:
        out += b">" + name.encode() + eol
        for i in range(0, len(s), width or max(len(s), 1)):
            out += s[i:i + (width or len(s))] + eol
    return out


def write_formats(d):
    """the same six reads in every format the reader takes -> {file name: the records as they stand in the decompressed file}"""
    fq, fq_crlf = ref.fastq_text(READS), ref.fastq_text(READS, b"\r\n")
    fa1, fa4, fa4_crlf = fasta_text(READS), fasta_text(READS, 4), fasta_text(READS, 4, b"\r\n")
    files = {"a.fq": fq, "b_crlf.fq": fq_crlf, "c.fa": fa1, "d_multi.fa": fa4, "e_multi_crlf.fa": fa4_crlf, "f.fq.gz": fq, "g.fa.gz": fa4, "h_noeol.fq": fq[:-1],
             "i_noeol.fa": fa4[:-1]}
    for fn, data in files.items():
        with (gzip.open(d / fn, "wb") if fn.endswith(".gz") else open(d / fn, "wb")) as f:
            f.write(data)
    return files


def records_of(data):
    """a file's records, split by this test: FASTQ four lines each, FASTA from each line that begins with > to the next"""
    lines = data.splitlines(keepends=True)
    if data[:1] == b"@":
        return [b"".join(lines[i:i + 4]) for i in range(0, len(lines), 4)]
    out = []
    for ln in lines:
        if ln[:1] == b">":
            out.append(b"")
        out[-1] += ln
    return out


def ref_counter(calls=None):
    def count(text, offs):
        assert text.dtype == np.uint8 and offs.dtype == np.int64 and offs[0] == 0 and offs[-1] == len(text)
        if calls is not None:
            calls.append(len(offs) - 1)
        m, p = ref.read_counts(ref.split(text.tobytes(), offs.tolist()), K, MD, PD, 1, 1)
        return np.array(m, dtype=np.uint32), np.array(p, dtype=np.uint32), 0.0
    return count


def expected(paths, paired=False, min_markers=1):
    n = len(paths)
    lens = [[len(s) for _, s in READS]] * n
    names = [[name.split()[0] for name, _ in READS]] * n
    m, p = ref.read_counts([s for _, s in READS], K, MD, PD, 1, 1)
    bins = ref.file_bins([m] * n, [p] * n, M_TOTAL, P_TOTAL, min_markers, paired)
    return ref.readbins_tsv(paths, lens, [m] * n, [p] * n, bins), ref.per_read_tsv(paths, names, lens, [m] * n, [p] * n, bins), bins


def test_reader_takes_every_format_and_the_writer_keeps_every_byte(tmp_path, monkeypatch):
    from jasper_amd import triobin
    files = write_formats(tmp_path)
    paths = [str(tmp_path / fn) for fn in files]
    m, p = ref.read_counts([s for _, s in READS], K, MD, PD, 1, 1)
    assert (m, p) == ([1, 0, 0, 1, 0, 0], [0, 2, 0, 1, 0, 0])      # r3: a maternal window in lower case, N, then a paternal one
    want_tsv, want_reads, bins = expected(paths)
    assert bins[0] == ["mat", "pat", "unknown", "pat", "unknown", "unknown"]      # r3: one window each, and the mother has more markers to show: 1 * 5 < 1 * 7
    for chunk in (16 << 20, 64, 7):                     # the parser's block size: whole files, and blocks that cut every record
        monkeypatch.setattr(triobin, "CHUNK", chunk)
        prefix = str(tmp_path / ("out%d" % chunk))
        per_bin, _ = triobin.bin_files(paths, prefix, ref_counter(), M_TOTAL, P_TOTAL, per_read=True, write_reads=True)
        assert open(prefix + ".readbins.tsv").read() == want_tsv
        assert open(prefix + ".readbins.reads.tsv").read() == want_reads
        assert per_bin == [(len(paths), 9 * len(paths)), (2 * len(paths), 25 * len(paths)), (3 * len(paths), 16 * len(paths))]
        for fn, data in files.items():
            recs = records_of(data)
            assert len(recs) == len(READS)
            base = fn[:-3] if fn.endswith(".gz") else fn
            got = {b: open("%s.%s.%s" % (prefix, b, base), "rb").read() for b in ref.BINS}
            for b in ref.BINS:                          # each record once, byte for byte, in input order
                assert got[b] == b"".join(r for r, rb in zip(recs, bins[0]) if rb == b), (fn, b, chunk)
            assert sum(len(g) for g in got.values()) == len(data)
        assert not [fn for fn in os.listdir(tmp_path) if fn.endswith(".tmp")]


def test_batches_are_cut_at_reads(tmp_path):
    from jasper_amd import triobin
    write_formats(tmp_path)
    paths = [str(tmp_path / "a.fq"), str(tmp_path / "d_multi.fa")]
    want_tsv, _, _ = expected(paths)
    for room, want_calls in ((1, [1] * 12), (19, [3, 2, 1, 3, 2, 1]), (1 << 20, [12])):      # 9 + 10 + 0 = 19 bytes fit a batch of 19, then 15 + 4, then 12
        calls = []
        prefix = str(tmp_path / ("b%d" % room))
        triobin.bin_files(paths, prefix, ref_counter(calls), M_TOTAL, P_TOTAL, batch_bases=room)
        assert calls == want_calls, room
        assert open(prefix + ".readbins.tsv").read() == want_tsv
        assert sorted(fn for fn in os.listdir(tmp_path) if fn.startswith("b%d." % room)) == ["b%d.readbins.tsv" % room]


def test_pairs_and_min_markers_in_the_files(tmp_path):
    from jasper_amd import triobin
    write_formats(tmp_path)
    paths = [str(tmp_path / "a.fq"), str(tmp_path / "c.fa")]
    for paired, mm in ((True, 1), (True, 3), (False, 2)):
        want_tsv, want_reads, _ = expected(paths, paired, mm)
        prefix = str(tmp_path / ("p%d%d" % (paired, mm)))
        triobin.bin_files(paths, prefix, ref_counter(), M_TOTAL, P_TOTAL, min_markers=mm, paired=paired, per_read=True)
        assert open(prefix + ".readbins.tsv").read() == want_tsv and open(prefix + ".readbins.reads.tsv").read() == want_reads


MALFORMED = [
    ("trunc.fq", ref.fastq_text(READS)[:-14], "record 5 is malformed: the file ends inside it"),
    ("trunc2.fq", ref.fastq_text(READS[:2]) + b"@r2\nACGT\n", "record 2 is malformed: the file ends inside it"),
    ("nohead.fq", ref.fastq_text(READS[:1]) + b"r1\nACGT\n+\nIIII\n", "record 1 is malformed: its first line does not begin with @"),
    ("noplus.fq", ref.fastq_text(READS[:3]) + b"@r3\nACGT\nACGT\nIIII\n", "record 3 is malformed: its third line does not begin with +"),
    ("qual.fq", b"@r0\nACGT\n+\nIII\n", "record 0 is malformed: its quality line is not as long as its sequence"),
    ("other.txt", b"ACGT\n", "record 0 is malformed: the file begins with neither @ (FASTQ) nor > (FASTA)"),
]


@pytest.mark.parametrize("name,data,message", MALFORMED)
def test_malformed_record_names_file_and_record_and_leaves_nothing(tmp_path, capsys, name, data, message):
    from jasper_amd import triobin
    write_formats(tmp_path)
    (tmp_path / name).write_bytes(data)
    before = set(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        triobin.bin_files([str(tmp_path / "a.fq"), str(tmp_path / name)], str(tmp_path / "out"), ref_counter(), M_TOTAL, P_TOTAL, per_read=True, write_reads=True)
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert str(tmp_path / name) in err and message in err
    assert set(os.listdir(tmp_path)) == before


def test_pair_with_unequal_record_counts_leaves_nothing(tmp_path, capsys):
    from jasper_amd import triobin
    (tmp_path / "R1.fq").write_bytes(ref.fastq_text(READS))
    (tmp_path / "R2.fq").write_bytes(ref.fastq_text(READS[:-1]))
    before = set(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        triobin.bin_files([str(tmp_path / "R1.fq"), str(tmp_path / "R2.fq")], str(tmp_path / "out"), ref_counter(), M_TOTAL, P_TOTAL, paired=True, write_reads=True)
    err = capsys.readouterr().err
    assert e.value.code == 1 and "--paired" in err and "R1.fq has 6 records" in err and "R2.fq has 5" in err
    assert set(os.listdir(tmp_path)) == before


# ---- flags: everything that is refused before a parent is opened (no GPU is touched: the tables come after the checks) --------------
def fake_jf(path, k):
    import json
    head = json.dumps({"key_len": 2 * k}).encode()
    path.write_bytes(b"%09d" % len(head) + head)


def test_flag_errors_exit_1_with_their_message_and_no_file(tmp_path, capsys, monkeypatch):
    from jasper_amd import triobin
    for fn in ("R1.fq", "R2.fq", "R3.fq", "mat.fq", "pat.fq"):
        (tmp_path / fn).write_bytes(ref.fastq_text(READS))
    os.mkdir(tmp_path / "sub")
    (tmp_path / "sub" / "R1.fq.gz").write_bytes(gzip.compress(ref.fastq_text(READS)))
    fake_jf(tmp_path / "m21.jf", 21)
    fake_jf(tmp_path / "p25.jf", 25)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr("jasper_amd.extensions.open_parents", lambda *a, **k: pytest.fail("a parent was opened"))
    parents = ["--mat", "mat.fq", "--pat", "pat.fq"]
    cases = [
        (["-r", "R1.fq", "--mat", "mat.fq"], "needs both parents"),
        (["-r", "R1.fq", "--mat", "mat.fq", "--mat-jf", "m21.jf", "--pat", "pat.fq"], "needs both parents"),
        (["-r", "R1.fq", "--mat", "gone.fq", "--pat", "pat.fq"], "--mat: a read file does not exist or is empty"),
        (["-r", "R1.fq", "--mat-jf", "m21.jf", "--pat-jf", "p25.jf"], "--pat-jf: the database's k is 25, the run's is 21"),
        (["-r", "R1.fq", "--mat-jf", "mat.fq", "--pat", "pat.fq"], "valid Jellyfish mer counts file"),
        (["-r", "R1.fq gone.fq"] + parents, "The reads file  gone.fq does not exist"),
        (parents, "No reads given"),
        (["-r", "R1.fq", "--mat-threshold", "0"] + parents, "integers of at least 1"),
        (["-r", "R1.fq", "--min-markers", "0"] + parents, "--min-markers takes an integer from 1 to"),
        (["-r", "R1.fq", "--min-markers", "two"] + parents, "--min-markers takes an integer from 1 to"),
        (["-r", "R1.fq", "--batch-bases", "0"] + parents, "--batch-bases takes an integer from 1 to"),
        (["-r", "R1.fq", "-k", "65"] + parents, "-k takes an integer from 1 to 64"),
        (["-r", "R1.fq R2.fq R3.fq", "--paired"] + parents, "--paired takes the read files as R1 R2 [R1 R2 ...]; 3 files were given"),
        (["-r", "R1.fq sub/R1.fq.gz", "--write-reads"] + parents, "would be written to the same files"),
    ]
    before = sorted(os.listdir(tmp_path))
    for argv, message in cases:
        with pytest.raises(SystemExit) as e:
            triobin.run(argv)
        assert e.value.code == 1, argv
        assert message in capsys.readouterr().err, argv
        assert sorted(os.listdir(tmp_path)) == before, argv
    with pytest.raises(SystemExit) as e:
        triobin.run(["--no-such-flag"])
    assert e.value.code == 1
    # the same two base names are fine when no read file is written: the check is --write-reads' own
    flags = triobin.check_flags(triobin.parse_args(["-r", "R1.fq sub/R1.fq.gz", "--mat-jf", "m21.jf", "--pat", "pat.fq", "--batch-bases", "300"]))
    assert flags[0] == ["R1.fq", "sub/R1.fq.gz"] and flags[1] == 21 and flags[4:] == (1, 300)      # (the database's header decides k)


def test_parents_without_hapmers_end_the_run(capsys):
    from jasper_amd import triobin
    for m, p, who in ((0, 5, "mother has"), (5, 0, "father has"), (0, 0, "parents have")):
        with pytest.raises(SystemExit) as e:
            triobin.check_totals(m, p)
        assert e.value.code == 1 and "The %s no hap-mers" % who in capsys.readouterr().err
    triobin.check_totals(1, 1)


# ---- the trio fixture is no vacuous input ------------------------------------------------------------------------------------------
def test_trio_fixture_separates_the_haplotypes():
    """asserted on the restatement alone, before any GPU comparison: at least 90 % of the child's reads go to mat or pat, both bins are
    used about equally, and the stretch without SNPs leaves reads in unknown"""
    t = ref.make_trio()
    k = ref.TRIO_K
    md, pd = ref.kmer_dict([t["hap_a"]], k, 4), ref.kmer_dict([t["hap_b"]], k, 4)
    mt, pt = ref.hapmer_total(md, pd, 2), ref.hapmer_total(pd, md, 2)
    assert mt > 1000 and pt > 1000
    for paired in (False, True):
        ms, ps = zip(*(ref.read_counts([s for _, s in t[f]], k, md, pd, 2, 2) for f in ("r1", "r2")))
        bins = [b for fb in ref.file_bins(ms, ps, mt, pt, 1, paired) for b in fb]
        n = len(bins)
        assert n == 2 * len(t["r1"]) > 3000
        assert bins.count("mat") + bins.count("pat") >= 0.9 * n and bins.count("unknown") >= 1
        assert bins.count("mat") > 0.4 * n and bins.count("pat") > 0.4 * n
