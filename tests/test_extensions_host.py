"""CPU: everything the two drivers do above the table for the extensions -- the driver's extension stage (cli._extensions) and
kmerqc.run -- on a FAKE table, against recordings of the code before the stage table (tests/recorded/extensions/*.json): every
written file byte for byte, the log messages, the `device seconds` lines, the labels of the `[timing]` lines, every call the table got
(method, thresholds, lengths, which table) and every table made and closed.

The fake's results are real result classes of jasper_amd/table.py with arrays of their dtypes, derived from the sequences they are
given, so that the input assembly and the polished FASTA differ; the polished FASTA lacks the second contig (report.align's None).
One difference from the recordings is allowed and asserted: each FASTA is parsed once, not once per stage function.
"""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from jasper_amd import cli, kmerqc, table as T      # noqa: E402

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recorded", "extensions")
K = 5
ASM = ">c1 first\nACGTTGCAAGCTTAGGCTAACGTAGCTAGGATCCATGCAAGT\nTTGACCAT\n>c2\nGGGATCCGATTTACGCATGCAAGCTTGGCACTGGCCGTCG\n>c3\nTTGACAGCTAGCTCAGTCCTAGGTATAATGCTAGCAACGTTCAGGCATCGAAGCTA\n"
POLISHED = ">c1\nACGTTGCAAGCTTAGGCTAACGTAGCTAGGATCCATGCAAGTTTGACCAT\n>c3\nTTGACAGCTAGCTCAGTCGTAGGTATAATGCTAGCAACGTTCAGCATCGAAGCTA\n"
HISTO = [(1, 100), (2, 50), (3, 20), (4, 10), (5, 5), (6, 8), (7, 30), (8, 60), (9, 40)]      # threshold 2, peak 8
HAP = ["--hapmers", "--mat", "mat.fq", "--pat", "pat.fq", "--mat-threshold", "3"]
CASES = {
    "report": ["--report"], "spectra": ["--spectra"], "copies": ["--copies"], "dups": ["--dups"], "variants": ["--variants"], "indels": ["--indels"],
    "compound": ["--compound"], "hapmers": HAP, "repair": ["--repair", "--repair-rounds", "2"],
    "compound_report": ["--compound", "--compound-max-len", "7", "--report"], "indels_variants": ["--indels", "--variants"],
    "indels_mixed_hets": ["--indels", "--indel-max-len", "3", "--indel-mixed", "--het-clusters", "--het-cluster-max-len", "8"],
    "copies_dups": ["--copies", "--dups", "--peak", "9", "--copies-min-run", "3", "--dups-min-run", "4"],
}
CASES["all"] = (["--report", "--spectra", "--copies", "--dups", "--variants", "--indels", "--indel-mixed", "--het-clusters", "--compound"] + HAP + ["--repair"])
RUNS = [("driver", c) for c in CASES] + [("kmerqc", c) for c in CASES if c not in ("repair", "compound_report")]      # (kmerqc: the report always, never a repair)


def _text(s):
    return s if isinstance(s, str) else bytes(s).decode("latin-1")


def _abc(s):
    s = _text(s)
    return s.count("A"), s.count("C"), s.count("G"), max(len(s) - K + 1, 0)


def _bases(n):
    return [n % 16, 0]


class FakeTable:
    """stands in for KmerTable: no GPU, fixed seconds, every call recorded in `events`"""
    events, serial, open_now, max_open = [], 0, 0, 0

    @classmethod
    def reset(cls):
        cls.events, cls.serial, cls.open_now, cls.max_open = [], 0, 0, 0

    def __init__(self, k, min_slots=1 << 20, device=0):
        cls = FakeTable
        cls.serial += 1
        cls.open_now += 1
        cls.max_open = max(cls.max_open, cls.open_now)
        self.k, self.device, self.n, self.text = int(k), device, cls.serial, ""
        cls.events.append(["new", self.n, self.k])

    @classmethod
    def from_jf(cls, path, device=0):
        return cls(K, device=device)

    def _call(self, name, *what):
        FakeTable.events.append([name, self.n] + [w.n if isinstance(w, FakeTable) else w for w in what])

    def close(self):
        FakeTable.open_now -= 1
        self._call("close")

    def count_files(self, files):
        self._call("count_files", [os.path.basename(f) for f in files])

    def count_bases(self, bases):
        self.text = _text(bases)
        self._call("count_bases", len(self.text))

    def histo_rows(self):
        self._call("histo_rows")
        return list(HISTO)

    def _report(self, seqs):
        counts, runs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((w, w, a % 7, c % 3))
            runs.append((a % 5, 1 + c % 4, c % 2, i, g % 3))
        return T.KmerReport(counts, np.array(runs, dtype=T.KMERRUN_DTYPE), 0.5, False)

    def kmer_report(self, seqs, thre):
        self._call("kmer_report", thre, [len(s) for s in seqs])
        return self._report(seqs)

    def spectrum(self, asm):
        self._call("spectrum", asm)
        cells = np.zeros((6, 10002), dtype=np.uint64)
        cells[0][5], cells[1][0], cells[1][2], cells[2][3] = 11, asm.text.count("C") % 13, len(asm.text) % 97, asm.text.count("A")
        return T.KmerSpectrum(cells, 0.25)

    def copy_report(self, asm, seqs, thre, peak):
        self._call("copy_report", asm, thre, peak, [len(s) for s in seqs])
        counts, runs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((w, w, a % 5, c % 4, a * peak, w))
            runs.append((g % 4, 3 + a % 5, a * 3, 3 + a % 5, i, 1 + c % 2))
        return T.CopyReport(counts, np.array(runs, dtype=T.COPYRUN_DTYPE), 0.125, False)

    def dup_map(self, asm, seqs, thre, peak):
        self._call("dup_map", asm, thre, peak, [len(s) for s in seqs])
        counts, runs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((w, w, a % 6, c % 3, g % 2, a % 2, a * 2))
            runs.append((a % 3, c % 3, 3 + g % 4, g * 2, c % 2, i, (i + 1) % len(seqs), a % 2, 0))
        return T.DupMap(counts, np.array(runs, dtype=T.DUPRUN_DTYPE), (0.0625, 0.03125), False)

    def _variants(self, seqs):
        counts, recs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            s = _text(s)
            counts.append((w, a % 4, c % 3))
            recs.append((g % len(s), i, 3, 4, ord(s[g % len(s)]), ord("A" if s[g % len(s)] != "A" else "C"), 1 + a % 2, 0))
        return T.VariantScan(counts, np.array(recs, dtype=T.VARIANT_DTYPE), sum(len(s) for s in seqs), 0.75, False)

    def variant_scan(self, seqs, thre):
        self._call("variant_scan", thre, [len(s) for s in seqs])
        return self._variants(seqs)

    def indel_scan(self, seqs, thre, max_len=4, mixed=False, clusters=0):
        self._call("indel_scan", thre, max_len, bool(mixed), clusters, [len(s) for s in seqs])
        counts, recs, mc, mr, hc, hr = [], [], [], [], [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((a % 3, c % 3, g % 3, a % 2))
            recs.append((2 + a % 5, i, 2, 5, 1 + c % 2, 1, ord("A"), 1 + g % 2, [0] * 7))
            recs.append((3 + c % 4, i, 1, 6, 1 + a % 2, 2, ord("C"), 1 + c % 2, [0] * 7))
            mc.append((a % 2, c % 2, 0))
            mr.append((4 + g % 3, i, 2, 7, a % 16, 2, 1 + a % 2, [0] * 5))
            hc.append((a % 4, c % 2, g % 2, 0))
            hr.append((1 + a % 4, i, 4, 5, 2, _bases(c), 2, [0] * 6))
        return T.IndelScan(counts, np.array(recs, dtype=T.INDEL_DTYPE), self._variants(seqs), 1.5, 0.5, 77, False,
                           T.MixedInsertions(mc, np.array(mr, dtype=T.MIXED_DTYPE), 0.375, 31, False) if mixed else None,
                           T.HetClusters(hc, np.array(hr, dtype=T.HET_CLUSTER_DTYPE), 0.4375, 19, False) if clusters else None)

    def compound_scan(self, seqs, thre, max_len=64):
        self._call("compound_scan", thre, max_len, [len(s) for s in seqs])
        counts, recs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((a % 4, c % 3, 1, g % 2, 0))
            recs.append((2 + g % 4, i, 1, 9, 1 + a % 2, _bases(a), 2, [0] * 6))
        return T.CompoundScan(counts, np.array(recs, dtype=T.COMPOUND_DTYPE), self._report(seqs), 2.5, 1.25, 41, False)

    def hapmer_scan(self, mat, pat, seqs, thre_mat, thre_pat, thre_child=1, child=True):
        self._call("hapmer_scan", mat, pat, thre_mat, thre_pat, thre_child, [len(s) for s in seqs])
        counts, runs = [], []
        for i, s in enumerate(seqs):
            a, c, g, w = _abc(s)
            counts.append((w, w, a % 5, c % 5))
            runs += [(a % 3, 2, i, 1), (10 + c % 3, 1 + g % 2, i, 2), (20 + g % 3, 1, i, 1)]
        return T.HapmerScan(counts, np.array(runs, dtype=T.HAPRUN_DTYPE), 0.625, False)

    def hapmer_census(self, mat, pat, asm=None, thre_mat=1, thre_pat=1, thre_child=1, child=True):
        self._call("hapmer_census", mat, pat, asm, thre_mat, thre_pat, thre_child)
        return T.HapmerCensus((100, len(asm.text) % 50, 7), (90, asm.text.count("A") % 40, 5), 0.875)

    def repair(self, seqs, thre, indel_max_len=4, compound_max_len=64, rounds=3):
        self._call("repair", thre, indel_max_len, compound_max_len, rounds, [len(s) for s in seqs])
        first = _text(seqs[0])
        y = "A" if first[5] != "A" else "C"
        new = [(first[:5] + y + first[6:]).encode()] + [_text(s).encode() for s in seqs[1:]]
        edits = np.zeros(1, dtype=T.EDIT_DTYPE)
        edits[0] = (5, 0, 1, 6, 1, ["ACGT".index(y), 0], 1, 1, 1, [0] * 4)
        before, after = self._report(seqs), self._report(new)
        return T.Repair(new, edits, [(1, 1, 0, 0, before.counts[0][2], after.counts[0][2])], before, after, 3.5, 0.1875)


def run_one(driver, case, tmp_path, monkeypatch, capsys):
    """one run in tmp_path -> what is compared: files, messages, device lines, timing labels, the table's events, the parses per text"""
    files = {"asm.fa": ASM, "asm.fa.polished.fasta": POLISHED, "threshold.txt": "2\n", "jfhisto%d.csv" % K: "".join("%d %d\n" % r for r in HISTO),
             "reads.fq": "@r\nACGT\n+\nIIII\n", "mat.fq": "@m\nACGT\n+\nIIII\n", "pat.fq": "@p\nACGT\n+\nIIII\n"}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("JASPER_AMD_TIMING", "1")
    mods = [cli, kmerqc, T]
    try:
        from jasper_amd import extensions
        mods.append(extensions)
    except ImportError:          # (the recordings were made before that module existed)
        pass
    for m in mods:
        monkeypatch.setattr(m, "KmerTable", FakeTable, raising=False)
    parses, real_read = {}, cli.read_assembly

    def counting_read(path, fast=True):
        parses[os.path.basename(path)] = parses.get(os.path.basename(path), 0) + 1
        return real_read(path, fast)
    monkeypatch.setattr(cli, "read_assembly", counting_read)
    monkeypatch.setattr(cli, "_T0", [0.0])
    FakeTable.reset()
    flags = CASES[case]
    capsys.readouterr()
    if driver == "driver":
        o = cli.parse_args(["-a", "asm.fa", "-r", "reads.fq", "-k", str(K)] + flags)
        reads = FakeTable(K)
        cli._extensions(cli._Ranks(), o, reads, "jfhisto%d.csv" % K, cli.hapmer_flags(o, K, None))
        reads.close()
    else:
        assert kmerqc.run(["-a", "asm.fa", "-r", "reads.fq", "-k", str(K), "-o", "out"] + [f for f in flags if f not in ("--report", "--repair")]) == 0
    out, err = capsys.readouterr()
    err = err.splitlines()
    return {"files": {p.name: p.read_text() for p in sorted(tmp_path.iterdir()) if p.name not in files},
            "messages": [ln.split("] ", 1)[1] for ln in out.splitlines() if re.match(r"^\[\w{3} \w{3} +\d", ln)],
            "device": [ln for ln in err if not ln.startswith("[timing")],
            "timing": [ln[len("[timing] "):].rsplit(None, 2)[0].rstrip() for ln in err if ln.startswith("[timing] ")],
            "events": FakeTable.events, "tables_made": FakeTable.serial, "tables_open_at_most": FakeTable.max_open, "parses": parses}


@pytest.mark.parametrize("driver,case", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_as_recorded(driver, case, tmp_path, monkeypatch, capsys):
    with open(os.path.join(RECORDED, "%s.%s.json" % (driver, case))) as f:
        want = json.load(f)
    got = run_one(driver, case, tmp_path, monkeypatch, capsys)
    assert sorted(got["files"]) == sorted(want["files"])
    for name in want["files"]:
        assert got["files"][name] == want["files"][name], name
    for what in ("messages", "device", "timing", "events", "tables_made", "tables_open_at_most"):
        assert got[what] == want[what], what
    # the one allowed difference: a text the recording parsed at all (once per stage function) is now parsed exactly once
    assert got["parses"] == {name: 1 for name in want["parses"]}

