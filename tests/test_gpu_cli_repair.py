"""GPU: `python -m jasper_amd.cli ... --repair` on the golden case homopolymer_k25 (its reads and its contig, written out as the driver's
inputs, as test_gpu_cli_compound.py does it) with ONE polishing pass: two passes of the walk leave no error record on any golden case,
one pass leaves this case seven (insertions, deletions and a mixed insertion).  The histogram of its small read set has no local minimum
(meta.json: jellyfish.py exits 1), so the case's own threshold is written to threshold.txt, which the driver then uses (src/jasper.sh:195-206).

With the flag the three new files and the new log line equal jasper_amd/repair.py's texts (checked on hand-made edits in
test_repair_host.py) of what the restatement of test_repair_host.py gives for the polished FASTA over a Python dict of the reads' k-mers;
the polished FASTA and every other file are what they are without it, also next to --report --compound --indels."""
import os

import pytest

from golden_util import Case
from test_gpu_cli_compound import K, write_inputs
from test_gpu_cli_spectra import cli, messages, read_fasta
from test_gpu_copies import dict_counter, kmer_dict
from test_repair_host import restate_repair

pytestmark = pytest.mark.gpu
REPAIR_FILES = ("asm.fa.repair.tsv", "asm.fa.repaired.fasta", "asm.fa.repairs.tsv")
OTHERS = ["--report", "--compound", "--indels"]
CASE = "homopolymer_k25"
ARGS = ["-r", "reads.fq", "-a", "asm.fa", "-k", str(K), "-t", "2", "-p", "1"]


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    out = {}
    for mode, flags in (("plain", []), ("repair", ["--repair"]), ("others", OTHERS), ("all", OTHERS + ["--repair", "--repair-rounds", "1"])):
        d = tmp_path_factory.mktemp(mode)
        write_inputs(d, CASE)
        with open(d / "threshold.txt", "w") as f:
            f.write("%d\n" % Case(CASE).thre)
        out[mode] = (d, cli(d, ARGS + flags))
    return out


def same_but(d0, d1, extra):
    """d1 holds d0's files byte for byte (the database's header holds the command line) and `extra`"""
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(extra) and set(os.listdir(d0)) <= set(os.listdir(d1))
    assert not [fn for fn in os.listdir(d1) if fn.endswith(".tmp")]
    for fn in sorted(set(os.listdir(d0)) - {"mer_counts%d.jf" % K}):
        if os.path.isfile(d0 / fn):
            assert open(d0 / fn, "rb").read() == open(d1 / fn, "rb").read(), fn


def expected(d, rounds):
    thre = int(open(d / "threshold.txt").read().split()[0])
    assert thre == Case(CASE).thre and Case(CASE).k == K
    count = dict_counter(kmer_dict(open(d / "reads.fq", "rb").read().split(b"\n")[1::4], K))
    names, pseqs = read_fasta(d / "asm.fa.polished.fasta")
    return names, pseqs, restate_repair(pseqs, K, count, thre, 4, 64, rounds)


def check_files(d, names, pseqs, want):
    from jasper_amd import repair
    final = [s.decode() for s in want["seqs"]]
    texts = [[s.decode() for s in t] for t in want["texts"]]
    polished = open(d / "asm.fa.polished.fasta", newline="").read()
    assert open(d / "asm.fa.repaired.fasta", newline="").read() == repair.fasta_text(polished, final)
    assert read_fasta(d / "asm.fa.repaired.fasta") == (names, final)
    assert open(d / "asm.fa.repairs.tsv").read() == repair.repairs_tsv_text(names, texts, want["edits"])
    assert open(d / "asm.fa.repair.tsv").read() == repair.repair_tsv_text(K, names, [len(s) for s in pseqs], [len(s) for s in final], want["edits"],
                                                                         want["before"][0], want["after"][0])
    return repair.log_text(K, want["rounds"], want["before"][0], want["after"][0])


def test_repair_files_and_log_line(runs):
    (d0, p0), (d1, p1) = runs["plain"], runs["repair"]
    names, pseqs, want = expected(d1, 3)
    assert len(want["edits"]) >= 1 and want["rounds"][0][5] < want["rounds"][0][4]      # the polished FASTA holds what the flag is for
    line = check_files(d1, names, pseqs, want)
    # without the flag: the same files but the three, byte for byte -- the polished FASTA among them -- and the same log lines but one
    same_but(d0, d1, REPAIR_FILES)
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    extra = [m for m in m1 if m.startswith("Repair:")]
    assert extra == [line] and [m for m in m1 if m not in extra] == m0
    assert m1.index(extra[0]) == len(m1) - 2 and m1[-1].startswith("Polished sequence is in")


def test_next_to_the_other_extensions(runs):
    """--report --compound --indels write what they write without --repair; --repair-rounds 1 stops after one round"""
    (d0, p0), (d1, p1) = runs["others"], runs["all"]
    same_but(d0, d1, REPAIR_FILES)
    names, pseqs, want = expected(d1, 1)
    assert len(want["rounds"]) == 1 and want["rounds"][0][1] >= 1
    line = check_files(d1, names, pseqs, want)
    m0, m1 = messages(p0.stdout), messages(p1.stdout)
    assert [m for m in m1 if m.startswith("Repair:")] == [line] and [m for m in m1 if not m.startswith("Repair:")] == m0
    # the polished FASTA is the one of a run without any extension
    assert open(d1 / "asm.fa.polished.fasta", "rb").read() == open(runs["plain"][0] / "asm.fa.polished.fasta", "rb").read()
