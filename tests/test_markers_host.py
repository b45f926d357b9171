"""CPU: the restatement the select and the assembly-mode tests compare with (tests/markers_ref.py) on dicts made by hand, the proof that
the assembly-mode fixture is no vacuous input -- asserted on the restatement alone -- and every refusal of `python -m jasper_amd.triobin`
that belongs to --hap1 / --hap2, each as a child process: none of them opens a file or touches a GPU."""
import json
import os
import subprocess
import sys

import pytest

import markers_ref as mr
import readbins_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2**32 - 1


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------------
def test_select_on_dicts_made_by_hand():
    src = {b"AAAAC": 1, b"AACCG": 2, b"ACGTA": 3, b"CCCCG": 7, b"AGAGA": 2**40}
    absent = {b"AACCG": 1, b"TTTTT": 9}
    solid = {b"AAAAC": 5, b"ACGTA": 1, b"AGAGA": 2**32 + 5, b"AACCG": 100}
    # no solid table: everything the other table does not hold
    assert mr.select(src, absent, None, 1, 1) == ({b"AAAAC": 1, b"ACGTA": 3, b"CCCCG": 7, b"AGAGA": 2**40}, (5, 1, 0, 4))
    # the source threshold comes first: a key below it is no candidate, whatever the other tables hold
    assert mr.select(src, absent, None, 3, 1) == ({b"ACGTA": 3, b"CCCCG": 7, b"AGAGA": 2**40}, (3, 0, 0, 3))
    assert mr.select(src, absent, None, 2, 1)[1] == (4, 1, 0, 3)
    # solid: absent from it is count 0; in_absent is counted before not_solid (AACCG is solid and still in_absent)
    assert mr.select(src, absent, solid, 1, 1) == ({b"AAAAC": 1, b"ACGTA": 3, b"AGAGA": 2**40}, (5, 1, 1, 3))
    assert mr.select(src, absent, solid, 1, 2) == ({b"AAAAC": 1, b"AGAGA": 2**40}, (5, 1, 2, 2))
    # the solid count is clamped to 2^32-1, which still meets a threshold of 2^32-1; the count that comes through is src's, whole
    assert mr.select(src, absent, solid, 1, U32) == ({b"AGAGA": 2**40}, (5, 1, 3, 1))
    # degenerate: nothing absent -> every candidate; absent = src -> nothing
    assert mr.select(src, {}, None, 1, 1) == (src, (5, 0, 0, 5))
    assert mr.select(src, dict(src), solid, 1, 1) == ({}, (5, 5, 0, 0))
    assert mr.select({}, absent, solid, 1, 1) == ({}, (0, 0, 0, 0))


def test_assembly_mode_truth_on_a_case_worked_by_hand():
    k = 5
    hap1, hap2 = [b"TTAACCGTT"], [b"TTAACAGTT"]        # one SNP: every window over it is private, 5 a side
    reads = {"a": [("r0", b"TAACCGT"), ("r1", b"TAACAGT"), ("r2", b"TTAAC"), ("r3", b"AACCG")], "b": [("s0", b"AACCGNAACAG")]}
    allm = mr.Haps(k, hap1, hap2, reads, "all")
    assert (allm.m_total, allm.p_total) == (4, 4) and allm.private == (4, 4)      # (TTAAC is shared; ACCGT is GGT.. canonical forms all differ)
    assert allm.m_stats == (5, 1, 0, 4)
    tsv, per_read, bins = allm.files(["a.fq", "b.fq"], ["a", "b"])
    assert bins == [["hap1", "hap2", "unknown", "hap1"], ["unknown"]]           # (s0: one marker of either side, a tie)
    assert allm.counts == {"a": ([3, 0, 0, 1], [0, 3, 0, 0]), "b": ([1], [1])}
    assert tsv.splitlines()[0] == "#file\tbin\treads\tbases\thap1_markers\thap2_markers"
    assert tsv.splitlines()[1:4] == ["a.fq\thap1\t2\t12\t4\t0", "a.fq\thap2\t1\t7\t0\t3", "a.fq\tunknown\t1\t5\t0\t0"]
    assert tsv.splitlines()[-3:] == ["*\thap1\t2\t12\t4\t0", "*\thap2\t1\t7\t0\t3", "*\tunknown\t2\t16\t1\t1"]
    assert per_read.splitlines()[0] == "#file\trecord\tname\tlength\thap1\thap2\tbin"
    assert per_read.splitlines()[1] == "a.fq\t0\tr0\t7\t3\t0\thap1" and per_read.splitlines()[-1] == "b.fq\t0\ts0\t11\t1\t1\tunknown"
    # solid at threshold 2: AACCG occurs 3 times in the reads, AACAG twice, every other private k-mer once
    solid = mr.Haps(k, hap1, hap2, reads, "solid", 2)
    assert (solid.m_total, solid.p_total) == (1, 1) and solid.private == (4, 4) and solid.m_stats == (5, 1, 3, 1)
    assert set(solid.m) == {b"AACCG"} and set(solid.p) == {ref.canonical(b"AACAG")}
    assert solid.files(["a.fq", "b.fq"], ["a", "b"])[2] == [["hap1", "hap2", "unknown", "hap1"], ["unknown"]]
    assert mr.Haps(k, hap1, hap2, reads, "solid", 3).p_total == 0


# ---- the fixture is no vacuous input -----------------------------------------------------------------------------------------------
def test_fixture_separates_the_haplotypes_and_the_errors_matter():
    """asserted on the restatement alone: with either marker set at least 90 % of the reads are binned and some stay unknown; hap1's
    assembly errors are markers under `all` and none under `solid`, so the totals differ, and at least one read changes its bin"""
    h = mr.make_haps()
    t = ref.make_trio()
    assert sum(a != b for a, b in zip(h["hap1"], t["hap_a"])) == len(range(700, len(t["hap_a"]), 1500)) >= 13 and h["hap2"] == t["hap_b"]
    reads = {"r1": h["r1"], "r2": h["r2"]}
    flat, totals = {}, {}
    for mode in ("all", "solid"):
        H = mr.Haps(ref.TRIO_K, [h["hap1"]], [h["hap2"]], reads, mode, mr.HAPS_THRE)
        bins = H.files(["R1.fq", "R2.fq"], ["r1", "r2"])[2]
        flat[mode], totals[mode] = bins[0] + bins[1], (H.m_total, H.p_total)
        n = len(flat[mode])
        print(mode, totals[mode], H.m_stats, H.p_stats, [flat[mode].count(b) for b in mr.BINS], n)
        assert n == 2 * len(h["r1"]) > 3000
        assert flat[mode].count("hap1") + flat[mode].count("hap2") >= 0.9 * n and flat[mode].count("unknown") >= 1
        assert H.m_total > 1000 and H.p_total > 1000
        assert H.private == totals["all"]
    assert totals["all"] != totals["solid"] and totals["solid"][0] < totals["all"][0]
    assert totals["all"][0] - totals["solid"][0] > totals["all"][1] - totals["solid"][1], "the errors are hap1's: its side loses more"
    assert sum(a != b for a, b in zip(flat["all"], flat["solid"])) >= 1


def test_histogram_rule_and_the_fixture_with_an_error_peak():
    """the rule restated, on histograms made by hand; the trio's reads alone derive no threshold, with the noise reads they derive 2"""
    hist = lambda rows: {("k%d_%d" % (m, i)): m for m, n in rows for i in range(n)}      # noqa: E731
    assert mr.histo_threshold(hist([(1, 50), (2, 20), (3, 5), (4, 2), (5, 9), (6, 30)])) == 2
    assert mr.histo_threshold(hist([(1, 50), (2, 20), (3, 5), (8, 5), (9, 4), (10, 30)])) == 4          # equal is no rise; rows need not be adjacent
    assert mr.histo_threshold(hist([(1, 50), (2, 20), (3, 30)])) is None                                # half of 2 is below 2
    assert mr.histo_threshold(hist([(1, 50), (2, 60)])) is None and mr.histo_threshold(hist([(1, 50), (2, 20), (7, 3)])) is None
    assert mr.histo_threshold({}) is None
    h = mr.make_haps()
    reads = [s for f in ("r1", "r2") for _, s in h[f]]
    assert mr.histo_threshold(ref.kmer_dict(reads, ref.TRIO_K)) is None
    child = ref.kmer_dict(reads + [s for _, s in mr.noise_reads()], ref.TRIO_K)
    assert mr.histo_threshold(child) == mr.HAPS_THRE == 2
    # the noise holds no k-mer of either haplotype: the markers are what they are without it
    with_noise = mr.Haps(ref.TRIO_K, [h["hap1"]], [h["hap2"]], {"r1": h["r1"], "r2": h["r2"], "noise": mr.noise_reads()}, "solid", 2)
    without = mr.Haps(ref.TRIO_K, [h["hap1"]], [h["hap2"]], {"r1": h["r1"], "r2": h["r2"]}, "solid", 2)
    assert with_noise.m == without.m and with_noise.p == without.p and with_noise.counts["noise"] == ([0] * 6, [0] * 6)


# ---- the refusals, each as a child process ----------------------------------------------------------------------------------------
def fake_jf(path, k):
    head = json.dumps({"key_len": 2 * k}).encode()
    path.write_bytes(b"%09d" % len(head) + head)


@pytest.fixture(scope="module")
def where(tmp_path_factory):
    d = tmp_path_factory.mktemp("haps_refused")
    for fn in ("R1.fq", "mat.fq", "pat.fq"):
        (d / fn).write_bytes(ref.fastq_text([("r0", b"TTAACCGTT")]))
    (d / "hap1.fa").write_bytes(mr.fasta(b"c1", b"TTAACCGTTACGATCGATCGGATC"))
    (d / "hap2.fa").write_bytes(mr.fasta(b"c1", b"TTAACAGTTACGATCGATCGGATC"))
    os.symlink(d / "hap1.fa", d / "hap1_again.fa")
    (d / "empty.fa").write_bytes(b"")
    fake_jf(d / "child.jf", 21)
    return d


HAPS = ["--hap1", "hap1.fa", "--hap2", "hap2.fa"]
REFUSED = [
    (["--hap1", "hap1.fa"], "--hap1 needs --hap2"),
    (["--hap2", "hap2.fa"], "--hap2 needs --hap1"),
    (HAPS + ["--mat", "mat.fq"], "--mat cannot be given with --hap1 / --hap2"),
    (HAPS + ["--pat-jf", "child.jf"], "--pat-jf cannot be given with --hap1 / --hap2"),
    (HAPS + ["--mat-threshold", "2"], "--mat-threshold cannot be given with --hap1 / --hap2"),
    (HAPS + ["--pat", "pat.fq", "--mat", "mat.fq"], "cannot be given with --hap1 / --hap2"),
    (["--hap1", "gone.fa", "--hap2", "hap2.fa"], "--hap1: gone.fa does not exist or is empty"),
    (["--hap1", "hap1.fa", "--hap2", "empty.fa"], "--hap2: empty.fa does not exist or is empty"),
    (["--hap1", "hap1.fa", "--hap2", "hap1.fa"], "--hap2: hap1.fa is the --hap1 assembly itself"),
    (["--hap1", "hap1.fa", "--hap2", "hap1_again.fa"], "--hap2: hap1_again.fa is the --hap1 assembly itself"),
    (HAPS + ["--markers", "weak"], "--markers takes solid or all; weak was given"),
    (["--mat", "mat.fq", "--pat", "pat.fq", "--markers", "all"], "--markers is an option of binning by two haplotype assemblies"),
    (["--mat", "mat.fq", "--pat", "pat.fq", "--child-threshold", "2"], "--child-threshold is an option of binning by two haplotype assemblies"),
    (["--mat", "mat.fq", "--pat", "pat.fq", "--child-jf", "child.jf"], "--child-jf is an option of binning by two haplotype assemblies"),
    (HAPS + ["--markers", "all", "--child-jf", "child.jf"], "--child-jf has no use with --markers all"),
    (HAPS + ["--markers", "all", "--child-threshold", "2"], "--child-threshold has no use with --markers all"),
    (HAPS + ["--child-threshold", "0"], "--child-threshold takes an integer from 1 to"),
    (HAPS + ["--child-threshold", "-1"], "--child-threshold takes an integer from 1 to"),
    (HAPS + ["--child-jf", "gone.jf"], "--child-jf: gone.jf does not exist or is empty"),
]


@pytest.mark.parametrize("args,message", REFUSED, ids=[" ".join(a) for a, _ in REFUSED])
def test_refusals_exit_1_name_the_flag_and_open_nothing(where, args, message):
    before = sorted(os.listdir(where))
    # (a GPU that is asked for does not exist: a run that got as far as a table would fail with another message)
    p = subprocess.run([sys.executable, "-m", "jasper_amd.triobin", "-r", "R1.fq", "--device", "1023", "--write-reads", "--per-read"] + args, cwd=where,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, p.stdout + p.stderr
    assert message in p.stderr, p.stderr
    assert sorted(os.listdir(where)) == before


def test_haplotypes_without_markers_end_the_run(capsys):
    from jasper_amd import triobin
    for m, p, who in ((0, 5, "hap1 has"), (5, 0, "hap2 has"), (0, 0, "The haplotypes have")):
        with pytest.raises(SystemExit) as e:
            triobin.haps_totals_check(m, p)
        assert e.value.code == 1 and "%s no marker k-mers" % who in capsys.readouterr().err
    triobin.haps_totals_check(1, 1)


def test_flags_of_assembly_mode_are_read(where, monkeypatch):
    from jasper_amd import triobin
    monkeypatch.chdir(where)
    flags = triobin.check_flags(triobin.parse_args(["-r", "R1.fq", "--marker-tables"] + HAPS))
    assert flags[1] == 37 and flags[3] == dict(hap1="hap1.fa", hap2="hap2.fa", markers="solid", thre_child=None, child_jf=None)
    flags = triobin.check_flags(triobin.parse_args(["-r", "R1.fq", "--child-jf", "child.jf", "--child-threshold", "3", "-k", "31"] + HAPS))
    assert flags[1] == 21 and flags[3]["thre_child"] == 3 and flags[3]["child_jf"] == "child.jf"      # (the database's header decides k)
    assert triobin.check_flags(triobin.parse_args(["-r", "R1.fq", "--markers", "all"] + HAPS))[3]["markers"] == "all"
    assert triobin.parse_args(["--marker-tables"])["marker_tables"] is True and triobin.parse_args([])["marker_tables"] is False
