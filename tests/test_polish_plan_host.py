"""CPU: jasper_amd/csrc/polish_plan.hpp -- everything a polishing lane computes on the host -- as a stand-alone program built with
-fsanitize=address,undefined (tools/polish_plan_check.cpp): case files in, lines out, `ok` at the end.  Nothing expected here
comes from the code under test: the cuts are those of the restated cut rule (tests/polish_plant.py: sync_candidates, clean_cells,
cuts), the segment fields follow from the cuts by the formulas polish_types.hpp documents, written out below, the bookkeeping is a
restatement of the prefix sums seg_summary_kernel documents, and the layout, the forced list and the record order are written out."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import polish_plant as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I31_MAX = 2**63 - 1, 2**31 - 1
GEO4 = {"TMIN": 1024, "CMIN": 32768, "CLEAN_CELL": 65536, "W": 16, "M": 12}       # test_polish_cuts_host.GEO: k = 4
ARENA_MSG = "polish: internal segment arena bound exceeded"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("plan") / "polish_plan_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "polish_plan_check.cpp"), "-o", out])
    return out


def run(exe, tmp_path, text, name="case.txt"):
    """the program's lines without the closing `ok`, each split into words"""
    path = tmp_path / name
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""]
    return [ln.split() for ln in lines[:-2]]


def join(*xs):
    return " ".join(str(int(x)) for x in xs)


def geo_of(k):
    g = P.geometry(k)
    assert (g["TMIN"], g["CMIN"], g["CLEAN_CELL"], g["W"], g["M"]) == (1024, 32768, 65536, 4 * k, 3 * k)      # the formulas below use these names
    return g


# ---- chunks -----------------------------------------------------------------------------------------------------------------------------
def _cls(n, bad=()):
    c = np.zeros(n, dtype=np.uint8)
    for a, b in bad:
        c[a:b] = P.BAD
    return c


def hand_chunks():
    """every case of test_polish_cuts_host.test_cuts_by_hand: (classes, length, cuts worked out by hand), k = 4"""
    k, T, CM = 4, GEO4["TMIN"], GEO4["CMIN"]

    def r(p):
        return (p, p + k)
    L, out = 6000, []
    n = L - k + 1
    out += [(_cls(n), L, []),
            (_cls(n, [r(2000), r(2000 + T)]), L, [(2000, 0), (2000 + T, 0)]),
            (_cls(n, [r(2000), r(1999 + T)]), L, [(2000, 0)]),
            (_cls(n, [r(2000), r(1999 + T), r(2020 + T)]), L, [(2000, 0), (2020 + T, 0)]),
            (_cls(n, [r(T - 1)]), L, []), (_cls(n, [r(T)]), L, [(T, 0)]),
            (_cls(n, [r(L - T)]), L, [(L - T, 0)]), (_cls(n, [r(L - T + 1)]), L, [])]
    L = 2 * T + k - 1
    out += [(_cls(2 * T, [r(T)]), L, []), (_cls(2 * T + 1, [r(T)]), L + 1, [(T, 0)])]
    L = 2 * CM + k - 1
    out += [(_cls(2 * CM), L, []), (_cls(2 * CM + 1), L + 1, [(CM, 1)])]
    L = 300_000
    n = L - k + 1
    out += [(_cls(n), L, [(32768, 1), (98304, 1), (163840, 1), (229376, 1)]),
            (_cls(n, [r(98304 - CM + 1)]), L, [(32768, 1), (98304 - CM + 1, 0), (163840, 1), (229376, 1)]),
            (_cls(n, [r(98304 + CM - 1)]), L, [(32768, 1), (98304 + CM - 1, 0), (163840, 1), (229376, 1)]),
            (_cls(n, [r(98304 + CM)]), L, [(32768, 1), (98304, 1), (98304 + CM, 0), (163840, 1), (229376, 1)]),
            (_cls(n, [r(98304 + CM + 1)]), L, [(32768, 1), (98304, 1), (98304 + CM + 1, 0), (229376, 1)])]
    for L, last in ((229376 + CM - 1, (163840, 1)), (229376 + CM, (229376, 1))):
        c = _cls(L - k + 1)
        want = P.cuts(c, L, k, GEO4)
        assert want[-1] == last
        out.append((c, L, want))
    out += [(_cls(0), 0, []), (_cls(0), k - 1, []), (_cls(4), k + 3, [])]
    return out


def fuzz_chunks(k, n, seed):
    """[(classes, length)]: lengths at and one either side of 2 TMIN + k - 1 and 2 CMIN + k - 1, up to several clean cells; BAD runs
    TMIN / CMIN -1, +0, +1 from the chunk start, the chunk end, each other and the cells' middles, and single BAD windows at the
    edges of what a clean-zone boundary needs clean"""
    g = geo_of(k)
    T, CM, CELL = g["TMIN"], g["CMIN"], g["CLEAN_CELL"]
    rng = np.random.default_rng(seed + k)
    lengths = [2 * T + k - 2, 2 * T + k - 1, 2 * T + k, 2 * CM + k - 2, 2 * CM + k - 1, 2 * CM + k, CELL + CELL // 2 + CM - 1, CELL + CELL // 2 + CM,
               CELL + CELL // 2 + CM + 1, 3000, 6000, 40_000, 150_000, 200_001, 300_000, 0, k - 1, k + 3]
    out = []
    for i in range(n):
        L = lengths[i % len(lengths)]
        nwin = max(0, L - k + 1)
        cls = np.zeros(nwin, dtype=np.uint8)
        menu = [(p, None) for p in (T - 1, T, T + 1, L - T - 1, L - T, L - T + 1)]
        if nwin > 2 * T + 8:
            base = int(rng.integers(T, nwin - T))
            menu += [(base, None), (base + int(rng.choice([T - 1, T, T + 1])), None)] * 2          # (twice: more likely both)
        for c in range(nwin // CELL + 1):
            mid = c * CELL + CELL // 2
            menu += [(mid + s * CM + d, None) for s in (-1, 1) for d in (-1, 0, 1)]
            menu += [(mid - 4 * k - 1, 1), (mid - 4 * k, 1), (mid + k - 1, 1), (mid + k, 1)]
        menu += [(int(p), None) for p in rng.integers(0, max(1, nwin), 3)]
        for p, r in menu:
            if rng.random() < (0.3, 0.1, 0.2, 0.05)[i // len(lengths) % 4]:     # (few runs: clean cuts survive; many: sync points crowd)
                r = r or int(rng.choice([k - 2, k - 1, k, k + 3]))
                if p >= 0 and p + r <= nwin:
                    cls[p:p + r] = P.BAD
        out.append((cls, L))
    return out


def batch_text(chunks, k, W, rng):
    """lengths, the candidates as the device lists them -- (chunk << 40) | position, shuffled -- and the cells per chunk"""
    words = [(c << 40) | p for c, (cls, _) in enumerate(chunks) for p in P.sync_candidates(cls, k, W)]
    words = [words[i] for i in rng.permutation(len(words))]
    cells = [P.clean_cells(cls, k, 65536) for cls, _ in chunks]
    return " ".join([join(len(chunks), *[L for _, L in chunks]), join(len(words), *words)] + [join(len(c), *c) for c in cells]), cells


def check_cuts(exe, tmp_path, chunks, k, geo, wants, name, hand=False):
    rng = np.random.default_rng(len(chunks) + k)
    head = "geometry %d %d %d %d\n" % (geo["TMIN"], geo["CMIN"], geo["W"], geo["M"]) if hand else ""
    text, cells = batch_text(chunks, k, geo["W"], rng)
    got = run(exe, tmp_path, head + "cuts %d 1 %s\ncuts %d 0 %s\n" % (k, text, k, text), name)
    assert len(got) == 4 * len(chunks)
    for i, ((cls, L), want) in enumerate(zip(chunks, wants)):
        line, sync = got[2 * i], got[2 * i + 1]
        assert line[0] == "cuts" and [(int(a), int(b)) for a, b in zip(line[1::2], line[2::2])] == want, (name, i, L)
        assert sync == ["sync", str(int(L - k + 1 > 2 * geo["TMIN"])), "cells", str(len(cells[i]))], (name, i)
        assert got[2 * len(chunks) + 2 * i] == ["cuts"], (name, i)                                 # speculate = false: no cuts
    return sum(len(w) for w in wants)


def test_cuts_by_hand_cases(exe, tmp_path):
    hand = hand_chunks()
    for cls, L, want in hand:
        assert P.cuts(cls, L, 4, GEO4) == want
    assert check_cuts(exe, tmp_path, [(c, L) for c, L, _ in hand], 4, GEO4, [w for _, _, w in hand], "hand.txt", hand=True) > 30


FUZZ_N = 72                                                                                    # per k: 216 chunks in all


@pytest.mark.parametrize("k", [4, 21, 37])
def test_cuts_fuzz(exe, tmp_path, k):
    g = geo_of(k)
    chunks = fuzz_chunks(k, FUZZ_N, 1000)
    wants = [P.cuts(cls, L, k, g) for cls, L in chunks]
    n = check_cuts(exe, tmp_path, chunks, k, g, wants, "fuzz%d.txt" % k)
    assert n > 80 and sum(1 for w in wants for _, ch in w if ch) >= 20 and sum(1 for w in wants for _, ch in w if not ch) > 30
    assert sum(1 for w in wants if not w) > 5


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
def al256(x):
    return (x + 255) // 256 * 256


def layout(lens, k, RM):
    """the arena layout written out: per chunk (cap, off_text, off_pos, off_cand, off_flag, off_cell, n_cells, cand_cap) and the totals"""
    T, W, M, CELL = 1024, 4 * k, 3 * k, 65536
    tot = dict(max_segs=0, text_bound=0, rec_bound=0, aux_bound=0, text=0, pos=0, cand=0, flag=0, cell=0)
    per = []
    for L in lens:
        cap = L + RM * max(4096, L // 8) + 64
        cand_cap = min(1 << 28, cap // (4 * k) + 16)
        n_cells = cap // CELL + 1
        per.append((cap, tot["text"], tot["pos"], tot["cand"], tot["flag"], tot["cell"], n_cells, cand_cap))
        tot["text"] += al256(cap)
        tot["pos"] += al256(cap)
        tot["cand"] += cand_cap
        tot["flag"] += al256((cap >> 6) + 2)
        tot["cell"] += n_cells
        ms = cap // T + 2                              # a segment per TMIN of text, and two
        tb = cap + ms * (W + M + 64)                   # the text with every segment's overlap
        tot["max_segs"] += ms
        tot["text_bound"] += tb + RM * (tb // 8 + ms * 1280)
        tot["rec_bound"] += RM * (2 * tb // k + 16 * ms)
        tot["aux_bound"] += RM * (2 * tb + 1024 * ms)
    return per, tot


def test_layout(exe, tmp_path):
    text, wants = "", []
    for k in (21, 37):
        lens = [0, 1, k - 1, 4095, 4096 * 8 - 1, 4096 * 8, 4096 * 8 + 1, 10**8]
        for RM in (1, 8):
            for ls in [[L] for L in lens] + [lens, []]:
                text += "layout %d %d %s\n" % (k, RM, join(len(ls), *ls))
                wants.append(layout(ls, k, RM))
    got = iter(run(exe, tmp_path, text))
    for per, t in wants:
        assert next(got) == ["layout"] + [str(t[x]) for x in ("max_segs", "text_bound", "rec_bound", "aux_bound", "text", "pos", "cand", "flag", "cell")]
        for p in per:
            assert next(got) == ["chunk"] + [str(x) for x in p]
    assert next(got, None) is None


# ---- segments ---------------------------------------------------------------------------------------------------------------------------
SEG_FIELDS = ("chunk first last chain_in seg_lo start_i stop_orig len0 len cap gs glen cls cls_n rec_cap edit_cap aux_cap own_lo own_hi own_hi0 "
              "buf recs edits aux arrive rest").split()


def segments_of(c, L, cuts, k, RM, tight, off_pos, cur, index):
    """the segments of chunk c from its cuts (polish_types.hpp, under SegDev); cur = [text, record, aux] cursors, moved on"""
    W, M = 4 * k, 3 * k
    m, out = len(cuts), []
    for j in range(m + 1):
        s = dict(chunk=c, first=int(j == 0), last=int(j == m), rest=0, gs=0)
        s["seg_lo"] = 0 if j == 0 else cuts[j - 1][0] - W
        s["start_i"] = 0 if j == 0 else W
        s["chain_in"] = 0 if j == 0 else cuts[j - 1][1]
        s["stop_orig"] = I64_MAX if j == m else cuts[j][0]
        hi = L if j == m else min(L, cuts[j][0] + M)
        s["len0"] = s["len"] = hi - s["seg_lo"]
        s["cap"] = s["len0"] + (2 if tight else RM * max(1024, s["len0"] // 8))
        s["glen"] = s["cap"] - s["len0"]
        s["cls"] = off_pos if L - k + 1 > 0 else -1
        s["cls_n"] = max(0, L - k + 1)
        s["rec_cap"] = s["edit_cap"] = min(I31_MAX, RM * (2 * s["len0"] // k + 16))
        s["aux_cap"] = min(I31_MAX, RM * (2 * s["len0"] + 1024))
        s["own_lo"] = 0 if j == 0 else 2 * k
        s["own_hi"] = s["own_hi0"] = -1 if j == m else cuts[j][0] - 2 * k - s["seg_lo"]
        s["buf"], s["recs"], s["edits"], s["aux"] = cur[0], cur[1], cur[1], cur[2]
        cur[0] += al256(s["cap"])
        cur[1] += s["rec_cap"]
        cur[2] += al256(s["aux_cap"])
        s["arrive"] = 1 + index + j
        out.append(s)
    return out


def parse_segs(lines):
    assert all(ln[0] == "seg" and len(ln) == len(SEG_FIELDS) + 1 for ln in lines)
    return [dict(zip(SEG_FIELDS, (int(x) for x in ln[1:]))) for ln in lines]


def check_disjoint(segs, tot):
    """text, record / edit and aux ranges of different segments are disjoint and inside their arenas"""
    for at, size, bound in (("buf", "cap", "text_bound"), ("recs", "rec_cap", "rec_bound"), ("edits", "edit_cap", "rec_bound"), ("aux", "aux_cap", "aux_bound")):
        spans = sorted((s[at], s[at] + s[size]) for s in segs)
        assert spans[0][0] >= 0 and spans[-1][1] <= tot[bound], at
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), at


def check_table(exe, tmp_path, chunks, k, RM, tight, failed, bounds, name):
    """one `table` command: the first table against the formulas, then the redo of `failed` behind it.  bounds = None (the layout's),
    or (which, delta): that bound of the redo is what the redo's cursor reaches, plus delta.  Returns (segments, the redo's verdict)."""
    g = geo_of(k)
    rng = np.random.default_rng(len(chunks) * 7 + k + RM)
    text, _ = batch_text(chunks, k, g["W"], rng)
    per, tot = layout([L for _, L in chunks], k, RM)
    cur, want, first = [0, 0, 0], [], []
    for c, (cls, L) in enumerate(chunks):
        first.append(len(want))
        want += segments_of(c, L, P.cuts(cls, L, k, g), k, RM, tight, per[c][2], cur, len(want))
    first.append(len(want))
    after = list(cur)
    want_redo = []
    for c in failed:
        want_redo += segments_of(c, chunks[c][1], [], k, RM, tight, per[c][2], cur, len(want_redo))
    b = [-1, -1, -1]
    if bounds:
        b[bounds[0]] = cur[bounds[0]] + bounds[1]
    got = run(exe, tmp_path, "table %d %d %d %s %s %s\n" % (k, RM, int(tight), text, join(len(failed), *failed), join(*b)), name)
    assert got[0] == ["table", "0", str(len(want))] + [str(x) for x in after] and got[1] == ["first"] + [str(x) for x in first]
    assert len(want) <= tot["max_segs"]
    segs = parse_segs(got[2:2 + len(want)])
    assert segs == want
    # whatever the formulas say: a chunk's owned ranges tile its text, and no two segments share arena space
    for c, (_, L) in enumerate(chunks):
        at = 0
        for s in segs[first[c]:first[c + 1]]:
            assert s["seg_lo"] + s["own_lo"] == at and (s["own_hi0"] == -1) == bool(s["last"])
            at = L if s["last"] else s["seg_lo"] + s["own_hi0"]
            assert 0 <= s["seg_lo"] and s["seg_lo"] + s["len0"] <= L and s["cap"] > s["len0"]
        assert at == L and segs[first[c]]["first"] and segs[first[c + 1] - 1]["last"] and sum(s["first"] for s in segs[first[c]:first[c + 1]]) == 1
    check_disjoint(segs, tot)
    assert [s["arrive"] for s in segs] == list(range(1, len(segs) + 1))
    # the redo
    limits = dict(tot)
    for i, key in enumerate(("text_bound", "rec_bound", "aux_bound")):
        if b[i] >= 0:
            limits[key] = b[i]
    room = cur[0] <= limits["text_bound"] and cur[1] <= limits["rec_bound"] and cur[2] <= limits["aux_bound"]
    head = got[2 + len(want)]
    assert head == ["redo", "0" if room else "-2", str(len(want_redo))] + [str(x) for x in cur], (name, head)
    redo = parse_segs(got[3 + len(want):])
    assert redo == want_redo and all(s["first"] and s["last"] and not s["chain_in"] for s in redo)
    if room and redo:
        check_disjoint(segs + redo, limits)
    return len(want), room


@pytest.mark.parametrize("k", [4, 21, 37])
def test_segments_fuzz(exe, tmp_path, k):
    chunks = fuzz_chunks(k, FUZZ_N, 1000)
    n, rooms = 0, []
    for RM, tight in ((1, False), (8, False), (1, True)):
        rng = np.random.default_rng(RM + k)
        for i in range(0, len(chunks), 6):
            group = chunks[i:i + 6]
            failed = [c for c in range(len(group)) if rng.random() < 0.4]
            got, room = check_table(exe, tmp_path, group, k, RM, tight, failed, None, "table_%d_%d_%d.txt" % (RM, tight, i))
            rooms.append(room or not failed)
            n += got
    # (the redo of a long chunk does not fit behind the table: the lane then redoes every chunk unsegmented; short ones fit)
    assert n > 3 * FUZZ_N + 200 and any(rooms) and not all(rooms)


@pytest.mark.parametrize("k", [21])
def test_redo_has_room_exactly_up_to_each_bound(exe, tmp_path, k):
    group = fuzz_chunks(k, 18, 1000)[10:16]
    for which in (0, 1, 2):
        assert check_table(exe, tmp_path, group, k, 1, False, [1, 4], (which, 0), "fits%d.txt" % which)[1]
        assert not check_table(exe, tmp_path, group, k, 1, False, [1, 4], (which, -1), "noroom%d.txt" % which)[1]
    assert check_table(exe, tmp_path, group, k, 1, False, [], (0, 0), "none.txt")[1]


# ---- rare-path bookkeeping ----------------------------------------------------------------------------------------------------------------
STATUS = {1: "text grew beyond its slack", 2: "fix-record buffer overflow", 3: "aux buffer overflow", 4: "path-extension scratch exhausted",
          5: "reference IndexError (src/jasper.py:221)", 6: "trial string too long"}


def book_table(rng, k=21):
    """three chunks of 1, 2 and 70 segments: lengths grown and shrunk, records and aux bytes on some"""
    segs = []
    for c, n in enumerate((1, 2, 70)):
        lo = 0
        for j in range(n):
            len0 = int(rng.integers(3000, 9000))
            d = int(rng.integers(-40, 41)) if rng.random() < 0.6 else 0
            nrec = int(rng.integers(0, 9)) if rng.random() < 0.5 else 0
            naux = int(rng.integers(1, 300)) if nrec and rng.random() < 0.5 else 0
            segs.append(dict(chunk=c, status=0, last=int(j == n - 1), len=len0 + d, len0=len0, own_lo=0 if j == 0 else 2 * k,
                             own_hi0=-1 if j == n - 1 else len0 - 5 * k, seg_lo=lo, nrec=nrec, naux=naux, lookups=int(rng.integers(0, 10**6)), wrong=int(rng.integers(0, 50))))
            lo += len0 - 7 * k
    return segs


def books(segs, n_chunks):
    """what seg_summary_kernel and seg_offsets_kernel document: per chunk running sums of the owned lengths, the length changes and the
    records; record and aux offsets run on through the chunks"""
    rows, newlen, nrec, naux = [], [0] * n_chunks, 0, 0
    shift, seqc = [0] * n_chunks, [0] * n_chunks
    for s in segs:
        c, d = s["chunk"], s["len"] - s["len0"]
        own_hi = s["len"] if s["last"] else s["own_hi0"] + d
        rows.append((own_hi, newlen[c], s["seg_lo"] + shift[c], seqc[c], nrec, naux))
        newlen[c] += own_hi - s["own_lo"]
        shift[c] += d
        seqc[c] += s["nrec"]
        nrec += s["nrec"]
        naux += s["naux"]
    return rows, newlen, nrec, naux


def books_text(segs, n_chunks, pass_i, passes):
    keys = "chunk status last len len0 own_lo own_hi0 seg_lo nrec naux lookups wrong".split()
    return "books %d %d %d %d %s\n" % (n_chunks, pass_i, passes, len(segs), " ".join(join(*[s[x] for x in keys]) for s in segs))


def test_rare_path_bookkeeping(exe, tmp_path):
    rng = np.random.default_rng(77)
    segs = book_table(rng)
    rows, newlen, nrec, naux = books(segs, 3)
    assert nrec > 50 and naux > 500 and any(s["len"] < s["len0"] for s in segs) and any(s["len"] > s["len0"] for s in segs)
    wrong = [sum(s["wrong"] for s in segs if s["chunk"] == c) for c in range(3)]
    variants = [(0, 2), (1, 2), (2, 2), (0, 0)]
    got = iter(run(exe, tmp_path, "".join(books_text(segs, 3, p, n) for p, n in variants)))
    for p, n in variants:
        assert next(got) == ["books", "0"]
        for r in rows:
            assert next(got) == ["b"] + [str(x) for x in r]
        assert next(got) == ["newlen"] + [str(x) for x in newlen]
        q0, q2 = (sum(wrong) if p == 0 else 0), (sum(wrong) if p == n else 0)
        assert next(got) == ["totals", str(nrec), str(naux), str(sum(s["lookups"] for s in segs)), str(q0), str(q2)]
        assert next(got) == ["qvchunk"] + [str(x) for c in range(3) for x in (wrong[c] if p == 0 else 0, wrong[c] if p == n else 0)]
    assert next(got, None) is None
    # one table per status that is not PS_OK: the message names the chunk, and only the reference's IndexError is -4
    text, wants = "", []
    for status, where in zip(sorted(STATUS), (0, 1, 2, 30, 72, 5)):
        bad = [dict(s) for s in segs]
        bad[where]["status"] = status
        text += books_text(bad, 3, 0, 2)
        wants.append((-4 if status == 5 else -2, "polish: chunk %d: %s" % (bad[where]["chunk"], STATUS[status])))
    got = run(exe, tmp_path, text, "status.txt")
    assert [(int(a[1]), " ".join(b[1:])) for a, b in zip(got[0::2], got[1::2])] == wants and all(a[0] == "books" and b[0] == "error" for a, b in zip(got[0::2], got[1::2]))


def test_chunk_totals_and_the_slack_check(exe, tmp_path):
    k, lens = 21, [0, 5, 20, 21, 50_000]
    per, _ = layout(lens, k, 1)
    caps = [p[0] for p in per]
    text, wants = "", []
    for p, n, newlen in ((0, 2, lens), (1, 2, lens), (2, 2, caps), (0, 0, caps), (0, 2, caps[:4] + [caps[4] + 1]), (2, 2, [caps[0] + 1] + caps[1:])):
        text += "chunks %d 1 %d %d %s\n" % (k, p, n, join(len(lens), *[x for pair in zip(lens, newlen) for x in pair]))
        tot = [L - k + 1 for L in lens]                   # src/jasper.py:51 counts len - k + 1 whatever its sign
        rc = -2 if any(a > b for a, b in zip(newlen, caps)) else 0
        wants.append((["chunks", str(rc), str(sum(tot) if p == 0 else 0), str(sum(tot) if p == n else 0)],
                      ["qvchunk"] + [str(x) for t in tot for x in (t if p == 0 else 0, t if p == n else 0)]))
    got = run(exe, tmp_path, text)
    assert [(a, b) for a, b in zip(got[0::2], got[1::2])] == wants and [w[0][1] for w in wants] == ["0", "0", "0", "0", "-2", "-2"]


# ---- the forced list, the records ------------------------------------------------------------------------------------------------------------
def test_forced_list_parser(exe, tmp_path):
    cases = [(3, '""', "-"), (3, "null", "-"), (3, '"all"', "1 1 1"), (3, '"0,2"', "1 0 1"), (3, '"2,,x"', "0 0 1"), (3, '"5,-1,1,3"', "0 1 0"), (3, '"x"', "0 0 0"),
             (3, '"1x,0"', "0 1 0"), (3, '"0,"', "1 0 0"), (3, '"alle"', "0 0 0"), (0, '"all"', "-"), (0, '"0"', "-"), (0, '""', "-"), (1, '"0"', "1"),
             (2, '"99999999999999999999,1"', "0 1")]
    got = run(exe, tmp_path, "".join("forced %d %s\n" % (n, s) for n, s, _ in cases))
    assert [" ".join(g) for g in got] == ["forced " + w for _, _, w in cases]


def test_regroup_and_sort(exe, tmp_path):
    rng = np.random.default_rng(5)
    X, S = ord("x"), ord("s")
    passes, recs = [], []                                     # recs: (chunk, pass, seqno, kind, bytes)
    for p in range(2):
        aux, lines, seq = b"", [], [0, 0]
        for c in (1, 0, 1, 1, 0, 0, 1, 0):                    # (the chunks interleaved; seqno rises inside a chunk)
            kind = X if rng.random() < 0.6 else S
            blob = bytes(rng.integers(0, 256, int(rng.integers(1, 12)), dtype=np.uint8)) if kind == X else b""
            patch = int(rng.integers(0, len(blob) + 1)) if blob else 0
            pad = bytes(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8))      # (bytes between two records' ranges: not theirs)
            aux += pad
            off = len(aux) if kind == X else 12345
            aux += blob
            lines.append(join(c, p, seq[c], kind, off, patch, len(blob) - patch if kind == X else 3))
            recs.append((c, p, seq[c], kind, blob))
            seq[c] += 1
        passes.append("%s %d %s" % (aux.hex() or "-", len(lines), " ".join(lines)))
    assert sum(1 for r in recs if r[3] == X and r[0] == 0) >= 3 and sum(1 for r in recs if r[3] == X and r[0] == 1) >= 3
    got = run(exe, tmp_path, "regroup 2 2 %s\n" % " ".join(passes))
    want, auxs = [], [b"", b""]
    for c, p, s, kind, blob in sorted(recs, key=lambda r: r[:3]):
        want.append(["rec", str(c), str(p), str(s), str(kind), str(len(auxs[c]) if kind == X else 12345)])
        auxs[c] += blob
    assert got == want + [["aux", a.hex()] for a in auxs]
