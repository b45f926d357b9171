"""CPU: the host half of the hap-mer evaluation (jasper_amd/hapmers.py) on hand-computed cases -- phase blocks, switches, N50, the
text of every file -- and the flag validation of kmerqc --hapmers, which must end the run before any table is made."""
import pytest

from jasper_amd import hapmers

MAT, PAT = 1, 2
K = 21


def blocks(markers, short_range=1000, max_switch_markers=3):
    return hapmers.phase_blocks(markers, K, short_range, max_switch_markers)


def B(start, end, kind, markers, kmers, sm=0, sk=0):
    return {"start": start, "end": end, "kind": kind, "markers": markers, "kmers": kmers, "switch_markers": sm, "switch_kmers": sk}


def test_a_lone_excursion_inside_the_range_is_a_switch():
    got = blocks([(0, 5, MAT), (100, 7, PAT), (300, 2, MAT)])
    assert got == [B(0, 300 + 2 + K - 1, MAT, 2, 7, 1, 7)]
    # two of them, closed by one return
    got = blocks([(0, 5, MAT), (100, 7, PAT), (150, 1, PAT), (300, 2, MAT), (400, 4, MAT)])
    assert got == [B(0, 400 + 4 + K - 1, MAT, 3, 11, 2, 8)]


def test_an_excursion_that_exceeds_the_short_range():
    # (1150 + 51) - 200 = 1001 > 1000: the block ends at its last own marker, the held-back markers start the next one
    got = blocks([(0, 5, MAT), (200, 7, PAT), (1150, 51, PAT), (1300, 2, MAT)])
    assert got == [B(0, 0 + 5 + K - 1, MAT, 1, 5), B(200, 1150 + 51 + K - 1, PAT, 2, 58), B(1300, 1300 + 2 + K - 1, MAT, 1, 2)]
    # exactly the range is still inside it
    got = blocks([(0, 5, MAT), (200, 7, PAT), (1150, 50, PAT), (1300, 2, MAT)])
    assert got == [B(0, 1300 + 2 + K - 1, MAT, 2, 7, 2, 57)]
    # one marker alone can exceed it
    got = blocks([(0, 5, MAT), (200, 1001, PAT), (1300, 2, MAT)])
    assert got == [B(0, 25, MAT, 1, 5), B(200, 1221, PAT, 1, 1001), B(1300, 1322, MAT, 1, 2)]
    # ... where the last one is a switch inside the second block when it is followed by that block's kind
    got = blocks([(0, 5, MAT), (200, 1001, PAT), (1300, 2, MAT), (1400, 3, PAT)])
    assert got == [B(0, 25, MAT, 1, 5), B(200, 1400 + 3 + K - 1, PAT, 2, 1004, 1, 2)]


def test_an_excursion_that_exceeds_max_switches():
    ms = [(0, 5, MAT), (10, 1, PAT), (20, 1, PAT), (30, 1, PAT)]
    assert blocks(ms + [(40, 2, MAT)]) == [B(0, 40 + 2 + K - 1, MAT, 2, 7, 3, 3)]                    # three are allowed
    got = blocks(ms + [(40, 1, PAT), (50, 2, MAT)])                                                   # the fourth is not
    assert got == [B(0, 25, MAT, 1, 5), B(10, 40 + 1 + K - 1, PAT, 4, 4), B(50, 50 + 2 + K - 1, MAT, 1, 2)]
    got = blocks(ms + [(40, 1, PAT), (50, 2, MAT), (60, 1, PAT)])
    assert got == [B(0, 25, MAT, 1, 5), B(10, 60 + 1 + K - 1, PAT, 5, 5, 1, 2)]


def test_an_excursion_never_closed_before_the_end():
    got = blocks([(0, 5, MAT), (50, 5, MAT), (100, 7, PAT), (150, 1, PAT)])
    assert got == [B(0, 50 + 5 + K - 1, MAT, 2, 10), B(100, 150 + 1 + K - 1, PAT, 2, 8)]


def test_one_marker_and_none():
    assert blocks([(17, 4, PAT)]) == [B(17, 17 + 4 + K - 1, PAT, 1, 4)]
    assert blocks([]) == []
    assert hapmers.block_n50([]) == 0
    assert hapmers.switch_rate_text(0, 0, 0) == "NA"


def test_defaults():
    ms = [(0, 5, MAT)] + [(10 + i, 1, PAT) for i in range(100)] + [(19000, 1000, MAT)]
    assert hapmers.phase_blocks(ms, K) == [B(0, 19000 + 1000 + K - 1, MAT, 2, 1005, 100, 100)]
    assert len(hapmers.phase_blocks(ms[:-1] + [(200, 1, PAT), (19000, 1000, MAT)], K)) == 3
    assert len(hapmers.phase_blocks([(0, 5, MAT), (10, 1, PAT), (20010, 1, PAT), (30000, 5, MAT)], K)) == 3
    assert (hapmers.SHORT_RANGE, hapmers.MAX_SWITCHES) == (20000, 100)


def test_n50_with_ties():
    mk = lambda *lens: [{"start": 0, "end": ln} for ln in lens]
    assert hapmers.block_n50(mk(10)) == 10
    assert hapmers.block_n50(mk(10, 10)) == 10
    assert hapmers.block_n50(mk(5, 5, 10)) == 10          # 10 holds exactly half
    assert hapmers.block_n50(mk(5, 6, 10)) == 6           # 10 < 10.5: the next one is needed
    assert hapmers.block_n50(mk(3, 3, 3, 3)) == 3
    assert hapmers.block_n50(mk(1, 2, 3, 4, 100)) == 100


def test_switch_rate_text():
    assert hapmers.switch_rate_text(3, 7, 7) == "50.0000"
    assert hapmers.switch_rate_text(2, 1005, 100) == "%.4f" % (100.0 * 100 / 1105) == "9.0498"
    assert hapmers.switch_rate_text(1, 4, 0) == "0.0000"
    assert hapmers.switch_rate_text(0, 0, 0) == "NA"


class Census:
    def __init__(self, mat, pat):
        self.mat, self.pat = mat, pat


def two_contigs():
    names, lengths = ["ctgA", "ctgB", "ctgC"], [2000, 500, 10]
    counts = [(1980, 1970, 14, 58), (480, 480, 4, 0), (0, 0, 0, 0)]
    runs = [(0, 0, 5, MAT), (0, 200, 7, PAT), (0, 1150, 51, PAT), (0, 1300, 2, MAT), (0, 1400, 7, MAT), (1, 17, 4, MAT)]
    return hapmers.Stage(K, names, lengths, counts, runs, 1000, 3)


def test_text_of_every_writer():
    st = two_contigs()
    assert st.blocks[0] == [B(0, 25, MAT, 1, 5), B(200, 1221, PAT, 2, 58), B(1300, 1427, MAT, 2, 9)] and st.blocks[2] == []
    assert hapmers.hapmers_tsv_text(st.names, [("asm", st)]) == (
        "#contig\tstage\tlength\twindows\tvalid\tmat\tpat\tmarkers\tblocks\tblock_n50\tswitch_markers\tswitch_kmers\tswitch_rate\n"
        "ctgA\tasm\t2000\t1980\t1970\t14\t58\t5\t3\t1021\t0\t0\t0.0000\n"
        "ctgB\tasm\t500\t480\t480\t4\t0\t1\t1\t24\t0\t0\t0.0000\n"
        "ctgC\tasm\t10\t0\t0\t0\t0\t0\t0\t0\t0\t0\tNA\n"
        "*\tasm\t2510\t2460\t2450\t18\t58\t6\t4\t1021\t0\t0\t0.0000\n")
    assert hapmers.bed_text(K, st.names, st.runs) == (
        "ctgA\t0\t25\tmat\t5\nctgA\t200\t227\tpat\t7\nctgA\t1150\t1221\tpat\t51\nctgA\t1300\t1322\tmat\t2\nctgA\t1400\t1427\tmat\t7\nctgB\t17\t41\tmat\t4\n")
    assert hapmers.blocks_bed_text(st.names, st.blocks) == (
        "ctgA\t0\t25\tmat\t1\t5\t0\t0\nctgA\t200\t1221\tpat\t2\t58\t0\t0\nctgA\t1300\t1427\tmat\t2\t9\t0\t0\nctgB\t17\t41\tmat\t1\t4\t0\t0\n")
    cen = Census((1000, 250, 300), (0, 0, 0))
    assert hapmers.completeness_text(K, 4, 5, 3, [("asm", cen)]) == (
        "#stage\thap\tk\tparent_threshold\tchild_threshold\thapmers\tfound\tcompleteness\toccurrences\n"
        "asm\tmat\t21\t4\t3\t1000\t250\t25.0000\t300\n"
        "asm\tpat\t21\t5\t3\t0\t0\tNA\t0\n")
    assert hapmers.stage_log_text(st, cen) == ("18 mat and 58 pat windows in 6 markers, 4 blocks (N50 1021), switch rate 0.0000; "
                                               "hap-mer completeness mat 25.0000 pat NA")


def test_before_and_after_rows_with_a_switch_and_a_missing_contig():
    before = two_contigs()
    after = hapmers.Stage(K, ["ctgB", "ctgA"], [501, 2000], [(481, 481, 4, 0), (1980, 1970, 21, 7)],
                          [(0, 17, 4, MAT), (1, 0, 5, MAT), (1, 200, 7, PAT), (1, 1300, 2, MAT), (1, 1400, 14, MAT)], 1000, 3)
    assert hapmers.hapmers_tsv_text(before.names, [("before", before), ("after", after)]) == (
        hapmers.TSV_HEADER +
        "ctgA\tbefore\t2000\t1980\t1970\t14\t58\t5\t3\t1021\t0\t0\t0.0000\n"
        "ctgA\tafter\t2000\t1980\t1970\t21\t7\t4\t1\t1434\t1\t7\t25.0000\n"
        "ctgB\tbefore\t500\t480\t480\t4\t0\t1\t1\t24\t0\t0\t0.0000\n"
        "ctgB\tafter\t501\t481\t481\t4\t0\t1\t1\t24\t0\t0\t0.0000\n"
        "ctgC\tbefore\t10\t0\t0\t0\t0\t0\t0\t0\t0\t0\tNA\n"
        "ctgC\tafter\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tNA\n"
        "*\tbefore\t2510\t2460\t2450\t18\t58\t6\t4\t1021\t0\t0\t0.0000\n"
        "*\tafter\t2501\t2461\t2451\t25\t7\t5\t2\t1434\t1\t7\t21.8750\n")
    assert hapmers.blocks_bed_text(after.names, after.blocks) == "ctgB\t17\t41\tmat\t1\t4\t0\t0\nctgA\t0\t1434\tmat\t3\t21\t1\t7\n"


def _no_tables(monkeypatch):
    from jasper_amd import cli, kmerqc

    class NoTable:
        def __init__(self, *a, **kw):
            raise AssertionError("a table was made before the flags were checked")

        from_jf = classmethod(lambda cls, *a, **kw: cls())

    monkeypatch.setattr(kmerqc, "KmerTable", NoTable)
    monkeypatch.setattr(cli, "KmerTable", NoTable)
    import jasper_amd.table
    monkeypatch.setattr(jasper_amd.table, "KmerTable", NoTable)
    return kmerqc


def _jf_stub(path, k):
    import json
    hdr = json.dumps({"format": "binary/sorted", "key_len": 2 * k, "counter_len": 4}).encode()
    hdr += b"\0" * (-(9 + len(hdr)) % 8)
    path.write_bytes(b"%09d" % len(hdr) + hdr + b"\0" * 16)
    return str(path)


@pytest.fixture()
def files(tmp_path):
    out = {}
    for name in ("asm.fa", "reads.fq", "mat.fq", "pat.fq"):
        (tmp_path / name).write_text(">x\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
        out[name] = str(tmp_path / name)
    out["mat21.jf"] = _jf_stub(tmp_path / "mat21.jf", 21)
    out["pat25.jf"] = _jf_stub(tmp_path / "pat25.jf", 25)
    out["run25.jf"] = _jf_stub(tmp_path / "run25.jf", 25)
    return out


BAD_FLAGS = [
    (["--mat", "mat.fq"], "give --hapmers as well"),
    (["--phase-short-range", "5"], "give --hapmers as well"),
    (["--pat-threshold", "5"], "give --hapmers as well"),
    (["--hapmers"], "needs both parents"),
    (["--hapmers", "--mat", "mat.fq"], "needs both parents"),
    (["--hapmers", "--pat", "pat.fq", "--mat", "mat.fq", "--mat-jf", "mat21.jf"], "exactly one of --mat"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "missing.fq"], "--pat: a read file does not exist"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--mat-threshold", "0"], "integers of at least 1"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--pat-threshold", "-3"], "integers of at least 1"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--pat-threshold", "x"], "integers of at least 1"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--phase-short-range", "0"], "integers of at least 1"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--phase-max-switches", "1.5"], "integers of at least 1"),
    (["--hapmers", "--mat-jf", "mat21.jf", "--pat", "pat.fq", "-k", "25"], "--mat-jf: the database's k is 21, the run's is 25"),
    (["--hapmers", "--mat", "mat.fq", "--pat-jf", "pat25.jf", "-k", "21"], "--pat-jf: the database's k is 25, the run's is 21"),
    (["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--threshold", "0"], "--hapmers needs a threshold of at least 1"),
]


@pytest.mark.parametrize("flags,message", BAD_FLAGS)
def test_kmerqc_refuses_bad_flags_before_any_table_is_made(monkeypatch, capsys, files, tmp_path, flags, message):
    kmerqc = _no_tables(monkeypatch)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        kmerqc.run(["-a", files["asm.fa"], "-r", files["reads.fq"]] + flags)
    assert e.value.code == 1
    assert message in capsys.readouterr().err


def test_the_runs_own_database_decides_k(monkeypatch, capsys, files, tmp_path):
    kmerqc = _no_tables(monkeypatch)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:            # -j run25.jf: the run's k is 25 whatever -k says
        kmerqc.run(["-a", files["asm.fa"], "-j", files["run25.jf"], "-k", "21", "--hapmers", "--mat-jf", "mat21.jf", "--pat-jf", "pat25.jf"])
    assert e.value.code == 1 and "--mat-jf: the database's k is 21, the run's is 25" in capsys.readouterr().err
    with pytest.raises(AssertionError, match="a table was made"):      # good flags: the run goes on to its first table
        kmerqc.run(["-a", files["asm.fa"], "-r", files["reads.fq"], "-k", "21", "--hapmers", "--mat-jf", "mat21.jf", "--pat", "pat.fq", "--mat-threshold", "2"])


def test_the_driver_takes_the_same_options(monkeypatch, capsys, files, tmp_path):
    from jasper_amd import cli
    monkeypatch.chdir(tmp_path)
    o = cli.parse_args(["-a", "asm.fa", "-r", "reads.fq", "--hapmers", "--mat", "mat.fq", "--pat-jf", "pat25.jf", "--mat-threshold", "7", "--phase-short-range", "500",
                        "--phase-max-switches", "9", "-k", "25"])
    got = cli.hapmer_flags(o, 25)
    assert got == {"mat": (["mat.fq"], None), "pat": (None, "pat25.jf"), "thre_mat": 7, "thre_pat": None, "short_range": 500, "max_switches": 9}
    assert cli.hapmer_flags(cli.parse_args(["-a", "asm.fa", "-r", "reads.fq"]), 25) is None
    with pytest.raises(SystemExit) as e:
        cli.hapmer_flags(cli.parse_args(["-a", "asm.fa", "--pat-jf", "pat25.jf"]), 25)
    assert e.value.code == 1 and "give --hapmers as well" in capsys.readouterr().err
