"""Repair stage: the writers of `*.repaired.fasta`, `*.repairs.tsv` and `*.repair.tsv` (cli --repair).

An extension: the reference repairs inside its walk and never looks again.  The scans of this package list what the walk has left;
their records of kind error -- a place where the contig's own k-mers are unreliable and the reads hold exactly one solid alternative --
all say "the reads hold the string y where the contig holds the R bytes from p on".  The stage (KmerTable.repair; semantics in
include/jasper_hip.h, jasper_repair) applies them on the GPU in rounds: scan, choose the edits that lie at least k - 1 bytes apart
(shorter edits first, then the better supported ones), rewrite the text, scan again.

Limits: het records are never applied (both alleles are in the reads); runs of unreliable k-mers longer than --compound-max-len and
complex sites stay as they are; edits that tie -- same place, same lengths, same support, another string -- are skipped.

Nothing here touches the GPU: the functions take names, sequences, edits, rounds and counters.
"""
from .report import contig_name, qv_text, totals, write_atomic  # noqa: F401  (every file of this module is written through write_atomic)

REPAIRS_HEADER = "#round\tcontig\tpos\tref\talt\tsource\trc\tac\n"
REPAIR_HEADER = ("#contig\tlength_polished\tlength_repaired\tsub\tins\tdel\tmixed\tcompound\tvalid_before\tunreliable_before\tQV_before\t"
                 "valid_after\tunreliable_after\tQV_after\n")
SOURCES = ("sub", "ins", "del", "mixed", "compound")


def _text(s):
    return s if isinstance(s, str) else bytes(s).decode("latin-1")


def fasta_text(polished_text, seqs):
    """the polished FASTA's text with the sequence of its i-th contig that has one replaced by seqs[i]: header lines, their order and
    the line layout stay; a contig whose sequence is unchanged keeps its lines byte for byte, a changed one is written on one line (as
    the join writes every contig)"""
    out, body, idx = [], [], 0

    def flush():
        nonlocal idx, body
        old = "".join(ln.rstrip("\n") for ln in body)
        if old:                                       # (a contig without a base is none of the sequences, as for every scan)
            new = _text(seqs[idx])
            idx += 1
            out.extend(body if old == new else [new + "\n"])
        else:
            out.extend(body)
        body = []

    for ln in polished_text.splitlines(keepends=True):
        if ln.startswith(">"):
            flush()
            out.append(ln)
        else:
            body.append(ln)
    flush()
    if idx != len(seqs):
        raise ValueError("repaired FASTA: %d sequences for %d contigs" % (len(seqs), idx))
    return "".join(out)


def round_texts(seqs, edits):
    """[the sequences round 1 read, the sequences round 2 read, ..]: `seqs` with the edits of the rounds before applied (one pass
    over a sequence per round, whatever the number of edits).  What `ref` of repairs_tsv_text is read from."""
    texts = [[_text(s) for s in seqs]]
    for rnd in sorted({e[0] for e in edits})[:-1]:
        by_seq = {}
        for e in edits:
            if e[0] == rnd:
                by_seq.setdefault(e[1], []).append(e)
        cur = list(texts[-1])
        for seq, es in by_seq.items():
            s, pieces, at = cur[seq], [], 0
            for _r, _s, pos, rlen, y, *_ in sorted(es, key=lambda e: e[2]):
                pieces += [s[at:pos], _text(y)]
                at = pos + rlen
            pieces.append(s[at:])
            cur[seq] = "".join(pieces)
        texts.append(cur)
    return texts


def repairs_tsv_text(names, texts, edits):
    """one line per applied edit (round, seq, pos, ref_len, y, source, ref_min, alt_min), ordered by (round, contig order, pos):
    round, contig, pos (0-based, in the coordinates of that round's input), ref = the replaced bytes as they stand in texts[round - 1]
    (`.` when empty), alt = y (`.` when empty), source, rc = ref_min, ac = alt_min.  texts[r] = the sequences that round r + 1 read."""
    out = [REPAIRS_HEADER]
    for rnd, seq, pos, rlen, y, source, rmin, amin in sorted(edits, key=lambda e: (e[0], e[1], e[2])):
        ref = _text(texts[rnd - 1][seq][pos:pos + rlen])
        out.append("%d\t%s\t%d\t%s\t%s\t%s\t%d\t%d\n" % (rnd, names[seq], pos, ref or ".", _text(y) or ".", source, rmin, amin))
    return "".join(out)


def repair_tsv_text(k, names, len_polished, len_repaired, edits, before, after):
    """one row per contig, then `*` with the sums: the two lengths, the applied edits by source, and valid / unreliable / QV of the
    dense report (windows, valid, unreliable, absent) before and after; QV as jasper_amd/report.py prints it"""
    per = [[0] * len(SOURCES) for _ in names]
    for e in edits:
        per[e[1]][SOURCES.index(e[5])] += 1
    out = [REPAIR_HEADER]

    def row(name, lp, lr, src, b, a):
        return "%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%s\n" % (name, lp, lr, "\t".join("%d" % n for n in src), b[1], b[2], qv_text(b[2], b[1], k), a[1], a[2],
                                                            qv_text(a[2], a[1], k))

    for i, name in enumerate(names):
        out.append(row(name, len_polished[i], len_repaired[i], per[i], before[i], after[i]))
    out.append(row("*", sum(len_polished), sum(len_repaired), [sum(p[j] for p in per) for j in range(len(SOURCES))], totals(before), totals(after)))
    return "".join(out)


def log_text(k, rounds, before, after):
    """`Repair: round 1: A records, B accepted, C conflicts, D ambiguous; ...; unreliable kmers X -> Y, dense QV Q0 -> Q1`"""
    b, a = totals(before), totals(after)
    parts = ["round %d: %d records, %d accepted, %d conflicts, %d ambiguous" % ((i + 1,) + tuple(r[:4])) for i, r in enumerate(rounds)]
    return "Repair: %s; unreliable kmers %d -> %d, dense QV %s -> %s" % ("; ".join(parts), b[2], a[2], qv_text(b[2], b[1], k), qv_text(a[2], a[1], k))
