"""CPU: jasper_amd/csrc/count_plan.hpp -- everything the counting path computes on the host -- as a stand-alone program built with
-fsanitize=address,undefined (tools/count_plan_check.cpp): case files in, lines out, `ok` at the end.  Nothing expected here comes
from the code under test: the geometry, the exchange's geometry and the piece sizes are the rules of the header's comments written
out again below, and next to them stand the invariants every result has to keep whatever the rules say.

One reading had to be chosen: "after restart_worst_case() the ratio is never trusted again" is asserted of the caller's size hint
(`have_ratio` stays false, and the piece after the restart is sized for the worst case); a ratio MEASURED on a later piece is
trusted again, as it is after any first piece."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, PIECE_MIN, PIECE_MAX, MAXBUCKETS, LI_MAXSL, BIG_LDS, HBINS = 16384, 8 << 20, 1 << 33, 2048, 64, 160 * 1024, 1024
KS = [16, 31, 32, 33, 37, 38, 48, 49, 64]
PIECES = [PIECE_MIN - 1, PIECE_MIN, 47_000_000, 1 << 30, 1 << 33]
OPT0 = dict(direct=0, no_rec16=0, no_wide=0, ngrp=0, nblk2=0, rb12=0, rb13=0, maxlists=0)
OPT_KEYS = ("direct", "no_rec16", "no_wide", "ngrp", "nblk2", "rb12", "rb13", "maxlists")
GEOM_KEYS = ("p1", "p2", "rbits", "recbits", "nblk1", "grid1", "nblk2", "cap1", "cap2")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("c++") is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("plan") / "count_plan_check")
    subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "jasper_amd", "csrc"),
                           os.path.join(ROOT, "tools", "count_plan_check.cpp"), "-o", out])
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


def opt(**kw):
    assert set(kw) <= set(OPT0)
    return dict(OPT0, **kw)


def opt_text(o):
    return " ".join(str(o[x]) for x in OPT_KEYS)


def min_log2_slots(k):
    """Table::min_log2_slots: the tag holds 53 remainder bits, the second word of a wide table 64 more"""
    return max(2 * k - 53 - 64, min(10, 2 * k))


# ---- the rules, written out ---------------------------------------------------------------------------------------------------------
def list_cap(avg):
    return int(min(4.0e9, avg * 1.25 + 8.0 * math.sqrt(avg) + 64.0))


def xchg_cap(avg, mult):
    """mean + 6 sigma, variance = mean x (1 + multiplicity)"""
    return int(min(4.0e9, avg + 6.0 * math.sqrt(avg * (1.0 + mult)) + 16.0))


def whole_lines(x):
    return (x + 15) // 16 * 16


def geometry(k, s, ext, piece, o):
    B = 2 * k
    if o["direct"] or piece < PIECE_MIN:
        return None
    rec16 = B > 74                                     # 8-byte records hold the hash below p1 <= 10 bucket bits
    if (rec16 and o["no_rec16"]) or (ext and not rec16) or (ext and o["no_wide"]):
        return None
    need = min(10, s - 12) if rec16 else max(0, B - 64)
    rg0 = 11 if ext else 12                            # regions of 2^12 slots, a wide table's of 2^11; one bit more only where the levels cannot split finer
    pick = None
    for maxp2 in ((9,) if rec16 else (9, 11)):         # first choice: at most 512 lists per bucket
        for rg in (rg0, rg0 + 1):
            p1 = max(need, int((s - rg + 1) / 2), 1)
            if p1 > 10 or p1 > s - 8:
                continue
            p2 = max(0, s - rg - p1)
            if p2 <= maxp2:
                pick = (p1, p2)
                break
        if pick:
            break
    if not pick:
        return None
    p1, p2 = pick
    ntiles = (piece + TILE - 1) // TILE
    grid1 = max(1, min(piece // ((1 << p1) * 512), ntiles, 256))
    nblk1 = min(grid1, o["ngrp"] or 8)
    tiles_per_slice = ((grid1 + nblk1 - 1) // nblk1) * ((ntiles + grid1 - 1) // grid1)
    avg1 = float(min(piece, tiles_per_slice * TILE)) / float(1 << p1)
    cap1 = int(min(4.0e9, avg1 * 1.10 + 8.0 * math.sqrt(avg1) + 64.0)) if avg1 >= 65536.0 else list_cap(avg1)
    nblk2 = max(1, min(nblk1, o["nblk2"] or (1 if (1 << p1) >= 256 else 8))) if p2 else 1
    cap2 = whole_lines(list_cap(float(piece) / (float(1 << (p1 + p2)) * float(nblk2)))) if p2 else 0
    return dict(p1=p1, p2=p2, rbits=s - p1 - p2, recbits=B - p1, nblk1=nblk1, grid1=grid1, nblk2=nblk2, cap1=cap1, cap2=cap2)


def xchg_geometry(k, s, piece_max, records_max, nown, o):
    """-> (p2b, geometry) or None"""
    if nown < 2 or nown > 8:
        return None
    piece_max = max(piece_max, PIECE_MIN)
    g = geometry(k, s, False, piece_max, o)
    if g is None or g["recbits"] > 64:
        return None
    rb13 = True if o["rb13"] else False if o["rb12"] else nown <= 4
    if g["p2"] > 0 and (nown << g["p2"]) > 512 and (nown << (g["p2"] - 1)) <= 512 and g["rbits"] == 12 and rb13:
        g["p2"] -= 1
        g["rbits"] += 1
    max_lists = max(2, o["maxlists"]) if o["maxlists"] else MAXBUCKETS
    p2b = 0
    while (nown << (g["p2"] - p2b)) > max_lists and p2b < g["p2"]:
        p2b += 1
    if (nown << (g["p2"] - p2b)) > MAXBUCKETS:
        return None
    g["p2"] -= p2b
    nb1 = 1 << g["p1"]
    g["nblk2"] = 1 if nb1 >= 256 else min(g["nblk1"], 8)
    if nown * g["nblk2"] > LI_MAXSL:
        return None
    lists = float(nb1) * float(nown << g["p2"]) * float(g["nblk2"])
    if records_max:
        rec = float(min(records_max, piece_max))
        keys = max(1.0, min(rec, 0.35 * float(1 << s) * float(nown)))
        g["cap2"] = xchg_cap(rec / lists, rec / keys)
    else:
        g["cap2"] = list_cap(float(piece_max) / lists)
    g["cap2"] = whole_lines(g["cap2"])
    return p2b, g


def window(pos, end, halo, misalign):
    start = max(0, pos - halo)
    start = max(0, start - (start + misalign) % 16)
    return start, end - start, pos - start


def next_piece(pos, n, first_new, distinct, nslots, mem_have, k, misalign, have_ratio, dup_ratio, override, started_empty):
    """(start, end, emit_from, expect_new, needs_room, histo_request, trusted)"""
    trusted = (pos > 0 or have_ratio) and dup_ratio < 0.6
    room = max(0, int(0.75 * float(nslots)) - distinct)
    piece = max(room, 1 << 20)
    if trusted:
        piece = max(piece, int(float(room) / max(0.05, 1.5 * dup_ratio)))
    if mem_have:
        piece = min(piece, max(mem_have // 28, 1 << 20))
    piece = min(piece, PIECE_MAX)
    if trusted and n - pos <= piece + piece // 4 and n - pos <= PIECE_MAX:
        piece = n - pos
    if have_ratio and pos == 0 and float(n) * dup_ratio <= float(room) and n <= PIECE_MAX and (not mem_have or n <= mem_have // 28):
        piece = n
    if override:
        piece = override
    todo = min(piece, n - pos)
    expect = int(float(todo) * min(1.0, dup_ratio)) if trusted else todo
    end = min(n, pos + piece)
    start, _, emit = window(pos, end, k - 1, misalign)
    histo = started_empty and pos == 0 and first_new == 0 and end == n and distinct == 0        # one piece, the whole input, into an empty table
    return start, end, emit, expect, int(expect > room and not override), int(histo), int(trusted)


def simulate(case):
    """the call the program's `walk` plays, played here: every piece brings ratio_ppm new keys per million new bases, the table grows
    by the growth rules (grow_at = 0.5), the ratio of a piece is what the next one is sized from.  -> the pieces, each with the
    planner's state before it (have_ratio, dup_ratio, distinct, s)"""
    k, s, n, first_new, mis, hint, mem, override, ratio, restart_at, distinct, occ, carried = case
    B = 2 * k
    started_empty = distinct == 0 and occ == 0
    have, dup = False, float(carried) / 1000000.0
    if hint > 0 and n > 1 << 24 and started_empty:           # the size hint stands in before anything has been measured
        dup = min(1.0, float(hint) / float(n))
        have = dup < 0.6
    pos, out = min(first_new, n), []
    while pos < n:
        start, end, emit, expect, needs_room, histo, trusted = next_piece(pos, n, first_new, distinct, 1 << s, mem, k, mis, have, dup, override, started_empty)
        out.append(dict(pos=pos, start=start, end=end, emit_from=emit, expect_new=expect, needs_room=needs_room, histo_request=histo, trusted=trusted, have_ratio=int(have),
                        dup_ratio=dup, distinct=distinct, s=s))
        assert end > pos and len(out) < 100000
        if needs_room:                                        # the worst case of what is coming kept under 3/4
            while distinct + expect > 0.75 * (1 << s) and s < B:
                s += 1
        if len(out) - 1 == restart_at:                        # cleared, two bits larger, worst-case sizing, from the start
            have, dup, distinct, occ, s, pos = False, 1.0, 0, 0, min(B, s + 2), min(first_new, n)
            continue
        occ_d = end - pos
        dist_d = occ_d * ratio // 10**6
        distinct += dist_d
        occ += occ_d
        if distinct > 0.5 * (1 << s) and s < B:               # past the load limit: to at most half of it
            s += 1
            while distinct > 0.25 * (1 << s) and s < B:
                s += 1
        dup = dist_d / occ_d                                  # new distinct keys per k-mer of the last piece
        pos = end
    return out, started_empty


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def geom_cases():
    out = []
    for k in KS:
        for s in range(min_log2_slots(k), 35):
            for ext in (0, 1):
                for piece in PIECES:
                    out.append((k, s, ext, piece, OPT0))
            # the switches, where they can matter
            for o in (opt(direct=1), opt(no_rec16=1), opt(no_wide=1), opt(ngrp=2), opt(ngrp=32), opt(nblk2=4)):
                for ext in (0, 1):
                    out.append((k, s, ext, 47_000_000, o))
    return out


def check_geometry(k, s, ext, piece, o, g):
    B = 2 * k
    assert g["p1"] + g["p2"] + g["rbits"] == s and g["recbits"] == B - g["p1"]
    assert g["recbits"] <= 64 or B > 74
    assert 1 <= g["p1"] <= 10 and 0 <= g["p2"] <= (9 if B > 74 else 11)
    rg0 = 11 if ext else 12
    if s - g["p1"] >= rg0:
        assert g["rbits"] in (rg0, rg0 + 1) and g["rbits"] in (11, 12, 13)
        if g["rbits"] == rg0 + 1:                          # the larger region only where the smaller one has no split: p1 <= 10, at most 512 lists per bucket
            q1 = max(min(10, s - 12) if B > 74 else max(0, B - 64), (s - rg0 + 1) // 2, 1)
            assert q1 > 10 or q1 > s - 8 or s - rg0 - q1 > 9
    else:
        assert g["p2"] == 0                                # one list level: the region is what the first level leaves
    assert g["cap2"] % 16 == 0 and (g["cap2"] > 0) == (g["p2"] > 0)
    assert 1 <= g["nblk1"] <= g["grid1"] <= 256 and 1 <= g["nblk2"] <= g["nblk1"]
    assert g["grid1"] <= (piece + TILE - 1) // TILE
    assert g["cap1"] >= piece / ((1 << g["p1"]) * g["nblk1"]) or g["cap1"] >= 3_999_999_999
    if g["p2"]:
        assert g["cap2"] >= piece / ((1 << (g["p1"] + g["p2"])) * g["nblk2"])


def test_geometry_is_the_restated_rule(exe, tmp_path):
    cases = geom_cases()
    got = run(exe, tmp_path, "".join("geom %d %d %d %d %s\n" % (k, s, ext, piece, opt_text(o)) for k, s, ext, piece, o in cases))
    assert len(got) == len(cases) > 3000
    taken = refused = 0
    for (k, s, ext, piece, o), ln in zip(cases, got):
        want = geometry(k, s, ext, piece, o)
        assert ln[0] == "geom" and int(ln[1]) == (want is not None), (k, s, ext, piece, o, ln)
        if want is None:
            refused += 1
            assert len(ln) == 2
            continue
        taken += 1
        g = dict(zip(GEOM_KEYS, map(int, ln[2:])))
        assert g == want, (k, s, ext, piece, o)
        check_geometry(k, s, ext, piece, o, g)
        # the refusals: a piece below 8 MiB, a wide table with 8-byte records, each switch
        assert piece >= PIECE_MIN and not o["direct"] and not (ext and 2 * k <= 74) and not (2 * k > 74 and o["no_rec16"]) and not (ext and o["no_wide"])
    assert taken > 1000 and refused > 1000
    by = {(k, s, ext, piece, opt_text(o)): ln for (k, s, ext, piece, o), ln in zip(cases, got)}
    # hand cases: bench.py's table, the smallest piece, one byte less; 16-byte records; a wide table; a table too small
    assert by[(31, 24, 0, PIECE_MIN, opt_text(OPT0))][1:5] == ["1", "6", "6", "12"]
    assert by[(31, 24, 0, PIECE_MIN - 1, opt_text(OPT0))] == ["geom", "0"]
    assert by[(37, 27, 0, 47_000_000, opt_text(OPT0))][1:6] == ["1", "10", "5", "12", "64"]          # B - 64 = 10 first-level bits
    assert by[(38, 27, 0, 47_000_000, opt_text(OPT0))][1:6] == ["1", "10", "5", "12", "66"]          # 16-byte records: as many first-level bits as there are
    assert by[(64, 27, 1, 47_000_000, opt_text(OPT0))][1:6] == ["1", "10", "6", "11", "118"]         # a wide table: regions of 2^11
    assert by[(31, 33, 0, 1 << 33, opt_text(OPT0))][1:5] == ["1", "10", "10", "13"]                   # nothing finer than 2^13 is left
    assert by[(31, 34, 0, 1 << 33, opt_text(OPT0))] == ["geom", "0"]                                  # (p1 would be 11)
    assert by[(16, 10, 0, 47_000_000, opt_text(OPT0))][1:5] == ["1", "1", "0", "9"]


def test_piece_buffers_launches_and_instances(exe, tmp_path):
    text, wants = "", []
    for p1, p2, recbits, nblk1, nblk2, ln in ((10, 5, 64, 8, 1, 47_000_000), (6, 0, 56, 8, 1, PIECE_MIN), (8, 7, 68, 8, 1, 48 * 65536 - 1), (8, 7, 68, 8, 1, 48 * 65537),
                                            (5, 4, 30, 4, 4, 1 << 33)):
        text += "bufs %d %d %d %d %d %d\n" % (p1, p2, recbits, nblk1, nblk2, ln)
        n1 = (1 << p1) * nblk1
        wants.append(["bufs", 1 << p1, 1 << (p1 + p2), n1, (1 << (p1 + p2)) * nblk2 if p2 else n1, 16 if recbits > 64 else 8, max(1 << 16, ln // 48)])
    for empty, ln in ((1, (1 << 32) - 1), (1, 1 << 32), (0, 100)):
        text += "fresh32 %d %d\n" % (empty, ln)
        wants.append(["fresh32", int(bool(empty) and ln < 1 << 32)])
    # the second pass: whole lines for up to 512 lists of whole-line slices; 16-byte records have no other kernel
    for recbits, p2, cap2, nown, own, old, kind in ((64, 5, 32, 1, 0, 0, "lines128"), (64, 7, 32, 1, 0, 0, "lines128"), (64, 8, 32, 1, 0, 0, "lines512"), (64, 9, 32, 1, 0, 0, "lines512"),
                                                   (64, 10, 32, 1, 0, 0, "general"), (64, 5, 40, 1, 0, 0, "general"), (64, 5, 32, 1, 0, 1, "general"), (64, 6, 32, 8, 1, 0, "owner_lines"),
                                                   (64, 7, 32, 8, 1, 0, "general_owner"), (64, 6, 32, 8, 1, 1, "general_owner"), (68, 9, 32, 1, 0, 0, "rec16_lines"),
                                                   (68, 9, 32, 1, 0, 1, "rec16_lines"), (68, 10, 32, 1, 0, 0, "none"), (68, 9, 24, 1, 0, 0, "none"), (64, 0, 0, 2, 1, 0, "owner_lines")):
        text += "part2 %d %d %d %d %d %d\n" % (recbits, p2, cap2, nown, own, old)
        wants.append(["part2", kind])
    # the insert: image bytes per slot 12 / 16 (fresh / loaded), a wide table's 20 / 24, the exchange's 16 + bins + slice offsets
    for rbits, nreg, ext, fresh, histo, xc in ((12, 1 << 15, 0, 1, 1, 0), (12, 1 << 15, 0, 1, 0, 0), (12, 1 << 15, 0, 0, 0, 0), (13, 1 << 21, 0, 0, 0, 0), (13, 1 << 21, 0, 1, 1, 0),
                                              (11, 1 << 16, 1, 1, 0, 0), (12, 1 << 16, 1, 0, 0, 0), (12, 1 << 16, 0, 1, 1, 1), (13, 1 << 16, 0, 0, 0, 1), (9, 2, 0, 1, 0, 0), (12, 700, 0, 1, 1, 0)):
        R = 1 << rbits
        lds = R * 16 + HBINS * 4 + (LI_MAXSL + 1) * 4 if xc else R * (20 if fresh else 24) if ext else R * (12 if fresh else 16) + (HBINS * 4 if histo else 0)
        text += "region %d %d %d %d %d %d\n" % (rbits, nreg, ext, fresh, histo, xc)
        wants.append(["region", lds, max(1, min(nreg, 256 * max(1, min(4, BIG_LDS // lds)) * 4))])
        assert lds <= BIG_LDS
    assert [w[1:] for w in wants if w[0] == "region"][:2] == [[4096 * 12 + 4096, 3072], [49152, 3072]]      # three workgroups per CU
    for ln, nslots, dirty in ((1 << 22, 1 << 24, 0), ((1 << 22) - 1, 1 << 24, 0), ((1 << 24) // 6, 1 << 24, 1), ((1 << 24) // 6 - 1, 1 << 24, 1)):
        text += "worth %d %d %d\n" % (ln, nslots, dirty)
        wants.append(["worth", int(ln >= (nslots // 6 if dirty else nslots // 4))])
    assert [w[1] for w in wants if w[0] == "worth"] == [1, 0, 1, 0]
    got = run(exe, tmp_path, text)
    assert got == [[str(x) for x in w] for w in wants]


# ---- exchange -------------------------------------------------------------------------------------------------------------------------
XCHG_TESTS = [(37, 2, 21, None), (37, 8, 21, None), (37, 4, 25, None), (25, 3, 21, None), (25, 2, 21, None), (31, 4, 22, None), (21, 8, 20, None), (25, 4, 25, 32), (37, 3, 25, 4),
              (31, 2, 24, 8)]                     # tests/test_gpu_exchange.py: k, ranks, log2 slots per shard, forced lists


def xchg_cases():
    out = []
    for k in (16, 31, 32, 33, 37, 38):
        for s in sorted(set(range(min_log2_slots(k), 35, 3)) | {21, 25, 32, 34}):
            for nown in range(2, 9):
                for piece in (PIECE_MIN, 47_000_000, 1 << 30):
                    for rec in (0, piece // 2, piece):
                        out.append((k, s, piece, rec, nown, OPT0))
                out += [(k, s, 1 << 30, 1 << 29, nown, opt(rb12=1)), (k, s, 1 << 30, 1 << 29, nown, opt(rb13=1))]
    for k, nown, s, maxlists in XCHG_TESTS:
        for piece in (1 << 20, 3_000_000, PIECE_MIN):
            for rec in (0, piece // 2, piece):
                out.append((k, s, piece, rec, nown, opt(maxlists=maxlists or 0)))
    out += [(31, 25, 1 << 30, 0, 1, OPT0), (31, 25, 1 << 30, 0, 9, OPT0), (31, 25, 1 << 30, 0, 4, opt(direct=1)), (31, 25, 1 << 30, 0, 4, opt(maxlists=1))]
    return out


def test_exchange_geometry_plan_and_owner_split(exe, tmp_path):
    cases = xchg_cases()
    # every owner derives its geometry from the same four numbers: the same command twice stands for two of them
    got = run(exe, tmp_path, "".join("xchg %d %d %d %d %d %s\n" % (k, s, piece, rec, nown, opt_text(o)) * 2 for k, s, piece, rec, nown, o in cases))
    assert got[0::2] == got[1::2] and len(got) == 2 * len(cases)
    n_ok = n_p2b = n_swap = n_forced = 0
    for (k, s, piece, rec, nown, o), ln in zip(cases, got[0::2]):
        want = xchg_geometry(k, s, piece, rec, nown, o)
        if want is None:
            assert ln == ["xchg", "-1"], (k, s, piece, rec, nown, o)
            continue
        n_ok += 1
        p2b, g = want
        bars = [i for i, w in enumerate(ln) if w == "|"]
        assert int(ln[1]) == p2b and dict(zip(GEOM_KEYS, map(int, ln[2:bars[0]]))) == g, (k, s, piece, rec, nown, o, ln)
        base = geometry(k, s, False, max(piece, PIECE_MIN), o)
        assert (nown << g["p2"]) <= 2048 and nown * g["nblk2"] <= LI_MAXSL and g["cap2"] % 16 == 0 and g["recbits"] <= 64
        assert g["p1"] + g["p2"] + p2b + g["rbits"] == s
        # the swap to 8192-slot regions: for up to four owners only, unless forced
        swapped = g["rbits"] == base["rbits"] + 1
        n_swap += swapped
        assert g["rbits"] in (base["rbits"], base["rbits"] + 1)
        if swapped:
            assert base["rbits"] == 12 and (nown << base["p2"]) > 512 and (nown <= 4 or o["rb13"]) and not (o["rb12"] and not o["rb13"])
        elif base["rbits"] == 12 and base["p2"] > 0 and (nown << base["p2"]) > 512 >= (nown << (base["p2"] - 1)):
            assert nown > 4 or o["rb12"]
        if p2b:
            n_p2b += 1
            limit = max(2, o["maxlists"]) if o["maxlists"] else 2048
            assert (nown << (g["p2"] + 1)) > limit >= (nown << g["p2"]) or g["p2"] == 0
        n_forced += bool(o["maxlists"]) and p2b > 0
        # the two cap formulas
        lists = (1 << g["p1"]) * (nown << g["p2"]) * g["nblk2"]
        pm = max(piece, PIECE_MIN)
        if rec:
            r = min(rec, pm)
            assert g["cap2"] >= r / lists + 6 * math.sqrt(r / lists) and g["cap2"] <= r / lists + 6.0 * math.sqrt(r / lists * (1 + r)) + 32
        else:
            assert g["cap2"] >= 1.25 * pm / lists
        # the eight words
        words = [int(x) for x in ln[bars[0] + 1:bars[1]]]
        lpo = 1 << (g["p1"] + g["p2"])
        assert words == [lpo * g["nblk2"] * g["cap2"], lpo * g["nblk2"], max(1 << 16, piece // 16), g["p1"], g["p2"] | (p2b << 8), g["rbits"], g["nblk2"], g["cap2"]]
        # the owner's second split and what its insert sees
        nreg, g2p1, g2p2, g2rec, g2nblk1, g2cap1, g2nblk2, g2cap2, gip1, gip2, girb, girec = [int(x) for x in ln[bars[1] + 1:]]
        assert nreg == 1 << (g["p1"] + g["p2"] + p2b) and nreg << g["rbits"] == 1 << s
        assert (g2p1, g2p2, g2rec) == (g["p1"] + g["p2"], p2b, g["recbits"] - g["p2"])
        assert (g2nblk1, g2cap1, g2nblk2) == (nown * g["nblk2"], g["cap2"], 1) and g2cap2 == list_cap(float(max(rec, 1)) / float(nreg))
        assert (gip1, gip2, girb, girec) == (g["p1"], g["p2"] + p2b, g["rbits"], g["recbits"]) and gip1 + gip2 + girb == s
    assert n_ok > 1500 and n_p2b >= 20 and n_swap >= 20 and n_forced >= 12
    # the forced cases of tests/test_gpu_exchange.py: the owner's extra pass exactly where lists are forced
    for k, nown, s, maxlists in XCHG_TESTS:
        p2b, g = xchg_geometry(k, s, 3_000_000, 0, nown, opt(maxlists=maxlists or 0))
        assert (p2b > 0) == bool(maxlists)
    # by hand: 2^25 slots, k = 25: 7 + 6 + 12 bits, 4 owners x 2^3 lists = 32; k = 37: 10 + 3 + 12, 3 owners x 2^0 <= 4; 2^24, k = 31: 6 + 6 + 12, 2 x 2^2 = 8
    by = {(c[0], c[1], c[2], c[3], c[4], c[5]["maxlists"]): ln for c, ln in zip(cases, got[0::2])}
    assert by[(25, 25, 3_000_000, 0, 4, 32)][1:5] == ["3", "7", "3", "12"] and by[(37, 25, 3_000_000, 0, 3, 4)][1:5] == ["3", "10", "0", "12"]
    assert by[(31, 24, 3_000_000, 0, 2, 8)][1:5] == ["4", "6", "2", "12"] and by[(37, 21, 3_000_000, 0, 8, 0)][1:5] == ["0", "10", "0", "11"]


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
PIECE_KEYS = ("pos", "start", "end", "emit_from", "expect_new", "needs_room", "histo_request", "trusted", "have_ratio", "dup_ratio", "distinct", "s")


def walk_cases():
    """k, s, n, first_new, misalign, hint, mem_have, override, ratio_ppm, restart_at, distinct0, occ0, carried_ppm"""
    out = []
    empty = (0, 0, 1_000_000)                    # an empty table whose planner has measured nothing yet
    ns = [1, 15, 16, 1000, (1 << 20) - 1, 1 << 20, (1 << 24) + 1, 47_000_000, 3 * (1 << 24) // 4, 3 * (1 << 24) // 4 + (8 << 20) + 2 * TILE + 7, (1 << 30) + 5, 1 << 33, (1 << 33) + 1,
          5 * (1 << 31) + 3, 1 << 35]
    for i, n in enumerate(ns):
        for k in (16, 31, 64):
            for s in (16, 20, 24, 27, 30):
                for first_new in (0, k - 1):
                    mis = (0, 1, 9, 15)[(i + s + first_new) % 4]
                    ratio = (50_000, 100_000, 400_000, 700_000, 1_000_000)[(i + k + s) % 5]
                    if k == 16:
                        ratio = min(ratio, (1 << 31) * 1_000_000 // max(n, 1 << 31))      # (no more keys than 4^16 / 2 exist)
                    hint = (0, n // 10, n // 3, int(n * 0.7))[(i + s // 2) % 4]
                    mem = (0, 200 << 30, 1 << 30)[(i + k) % 3]
                    out.append((k, s, n, first_new, mis, hint, mem, 0, ratio, -1) + empty)
    for mis in (0, 1, 9, 15):                    # every misalignment on one multi-piece call, with and without a hint and the memory bound
        for hint in (0, 2_000_000):
            for mem in (0, 28 * (3 << 20)):
                out.append((37, 24, 60_000_000, 0, mis, hint, mem, 0, 90_000, -1) + empty)
                out.append((37, 24, 60_000_000, 36, mis, hint, mem, 0, 90_000, -1) + empty)
    # the size-hint restart: a hint that promised a repetitive input, a piece sized from it, the restart after it
    out += [(31, 22, 40_000_000, 0, 9, 1_000_000, 0, 0, 600_000, 0) + empty, (31, 22, 40_000_000, 30, 0, 1_000_000, 0, 0, 100_000, 0) + empty,
            (31, 24, 100_000_000, 0, 1, 3_000_000, 0, 0, 1_000_000, 0) + empty]
    # JASPER_EXPERIMENT_PIECE
    out += [(31, 20, 10_000_000, 0, 9, 0, 0, 1 << 21, 1_000_000, -1) + empty, (31, 20, 10_000_000, 0, 0, 500_000, 0, 3_000_001, 100_000, -1) + empty,
            (31, 24, 1 << 31, 30, 15, 0, 1 << 30, 1 << 29, 50_000, -1) + empty]
    return out + filled_cases()


def filled_cases():
    """calls into a table that is not empty, or whose planner carries a ratio from the call before: the hint is ignored, no histogram
    is fused even into one piece that is the whole input, and the carried ratio is trusted from the first piece on only when context
    lies before it (pos > 0)"""
    n1 = (1 << 24) + 5                           # one piece into 2^26 slots, long enough for a hint to count
    return [(31, 26, n1, 0, 0, 1_000_000, 0, 0, 100_000, -1, 1000, 5000, 1_000_000),        # filled: hint ignored, whole input in one piece, no histogram
            (31, 26, n1, 0, 0, 1_000_000, 0, 0, 100_000, -1, 0, 7, 1_000_000),              # occurrences without a key (all spilled, say): not empty either
            (31, 26, n1, 0, 0, 1_000_000, 0, 0, 100_000, -1, 0, 0, 1_000_000),              # the same call into the empty table: hint and histogram
            (31, 26, n1, 0, 0, 0, 0, 0, 100_000, -1, 0, 0, 100_000),                        # empty, no hint, a ratio carried: not trusted at pos 0, histogram
            (31, 24, 60_000_000, 30, 9, 2_000_000, 0, 0, 80_000, -1, 3_000_000, 30_000_000, 100_000),      # carried ratio, context before the first piece: trusted at once
            (31, 24, 60_000_000, 0, 9, 2_000_000, 0, 0, 80_000, -1, 3_000_000, 30_000_000, 100_000),       # ... none: worst case first
            (31, 24, 60_000_000, 30, 1, 2_000_000, 0, 0, 80_000, -1, 3_000_000, 30_000_000, 700_000),      # a carried ratio that is not below 0.6
            (37, 22, 200_000_000, 36, 15, 0, 1 << 30, 0, 30_000, -1, 2_000_000, 90_000_000, 20_000),       # nearly full, memory bound, the table grows up front
            (31, 24, 40_000_000, 0, 0, 1_000_000, 0, 1 << 22, 500_000, -1, 500_000, 500_000, 1_000_000)]   # filled, JASPER_EXPERIMENT_PIECE


def test_pieces_of_simulated_calls(exe, tmp_path):
    cases = walk_cases()
    got = iter(run(exe, tmp_path, "".join("walk " + " ".join(str(x) for x in c) + "\n" for c in cases)))
    seen = dict(trusted=0, tail_rule=0, histo=0, needs_room=0, multi=0, mem_bound=0, restarted=0, capped=0, override=0, measured=0, grown=0)
    for case in cases:
        k, s0, n, first_new, mis, hint, mem, override, ratio, restart_at, distinct0, occ0, carried = case
        pieces = []
        for ln in got:
            if ln[0] == "walked":
                assert int(ln[1]) == len(pieces)
                break
            assert ln[0] == "piece" and len(ln) == len(PIECE_KEYS) + 1
            p = dict(zip(PIECE_KEYS, ln[1:]))
            pieces.append({x: (float(v) if x == "dup_ratio" else int(v)) for x, v in p.items()})
        # every number of every piece, the planner's state before it included, is what the call played in Python gives
        want, started_empty = simulate(case)
        assert len(pieces) == len(want), case
        for i, (p, w) in enumerate(zip(pieces, want)):
            assert p == w, (case, i, p, w)
        if min(first_new, n) == n:                                          # nothing but context
            assert not pieces, case
            continue
        assert pieces, case
        seen["multi"] += len(pieces) > 2
        seen["measured"] += len({p["dup_ratio"] for p in pieces}) > 2
        seen["grown"] += pieces[-1]["s"] > s0
        # whatever the rules say
        at = min(first_new, n)
        restarted = False
        for i, p in enumerate(pieces):
            ctx = (case, i, p)
            assert p["pos"] == at, ctx                                     # in order, each base once
            assert p["pos"] < p["end"] <= n
            assert p["start"] == 0 or (p["start"] + mis) % 16 == 0, ctx
            assert p["emit_from"] == p["pos"] - p["start"] and p["emit_from"] >= min(p["pos"], k - 1) and p["emit_from"] <= k - 1 + 15, ctx
            if override:
                assert p["end"] - p["pos"] == min(override, n - p["pos"]) and not p["needs_room"], ctx
                seen["override"] += 1
            else:
                assert p["end"] - p["pos"] <= PIECE_MAX, ctx
                seen["capped"] += p["end"] - p["pos"] == PIECE_MAX
                if p["trusted"] and p["end"] < n and n - p["pos"] <= PIECE_MAX:
                    assert n - p["end"] > (p["end"] - p["pos"]) // 4, ctx        # no small tail for a launch of its own
                if p["trusted"] and p["end"] == n and i > 0:
                    seen["tail_rule"] += 1
                if mem and not p["trusted"]:
                    assert p["end"] - p["pos"] <= max(mem // 28, 1 << 20), ctx
                seen["mem_bound"] += bool(mem) and p["end"] - p["pos"] == max(mem // 28, 1 << 20)
            if p["histo_request"]:
                assert started_empty and p["pos"] == 0 and first_new == 0 and p["end"] == n and p["distinct"] == 0 and distinct0 == 0 and occ0 == 0, ctx
                seen["histo"] += 1
            if not p["have_ratio"] and p["pos"] == 0:
                assert not p["trusted"], ctx                                # a carried or measured ratio needs context before the piece
            if p["have_ratio"]:
                assert hint > 0 and started_empty and not restarted, ctx     # only the hint, only into an empty table
            if p["needs_room"]:
                assert p["expect_new"] > int(0.75 * (1 << p["s"])) - p["distinct"], ctx
            seen["needs_room"] += p["needs_room"]
            seen["trusted"] += p["trusted"]
            if restarted:
                assert not p["have_ratio"], ctx                             # the hint is never trusted again
            if i == restart_at:
                assert p["have_ratio"] and p["trusted"] and not p["needs_room"], ctx      # (the case is what it was meant to be)
                restarted = True
                at = min(first_new, n)
                nxt = pieces[i + 1]
                assert (nxt["have_ratio"], nxt["trusted"], nxt["dup_ratio"], nxt["distinct"], nxt["s"]) == (0, 0, 1.0, 0, min(2 * k, p["s"] + 2)), ctx
                assert nxt["expect_new"] == nxt["end"] - nxt["pos"]          # worst case: every base a new key
                seen["restarted"] += 1
            else:
                at = p["end"]
        assert at == n, case                                                # the pieces end where the input ends
        assert sum(p["histo_request"] for p in pieces) <= 1 + (restart_at >= 0)
    assert next(got, None) is None
    assert seen["trusted"] > 200 and seen["tail_rule"] > 20 and seen["histo"] > 50 and seen["needs_room"] > 20 and seen["multi"] > 100, seen
    assert seen["mem_bound"] > 5 and seen["restarted"] == 3 and seen["capped"] >= 2 and seen["override"] > 10 and seen["measured"] > 50 and seen["grown"] > 100, seen


def test_filled_tables_by_hand(exe, tmp_path):
    """the first piece of each call of filled_cases, worked out by hand: (have_ratio, dup_ratio, trusted, histo_request, end - pos;
    None: a quotient whose last digit is the floating point's, left to the walk above)"""
    n1 = (1 << 24) + 5
    room24 = 3 * (1 << 24) // 4 - 3_000_000      # 9 582 912 free slots under 3/4
    assert n1 < 3 * (1 << 26) // 4 - 1000
    wants = [(0, 1.0, 0, 0, n1),                 # filled: the hint is ignored, no histogram; the room of 50 M takes the whole input
             (0, 1.0, 0, 0, n1),                 # occurrences without keys: the same
             (1, 1_000_000 / n1, 1, 1, n1),      # empty: the hint's ratio, one piece, the histogram fused
             (0, 0.1, 0, 1, n1),                 # a carried ratio is not trusted at pos 0; the table is empty: histogram
             (0, 0.1, 1, 0, 60_000_000 - 30),    # trusted: the room / 0.15 = 63.9 M, more than what is left: all of it
             (0, 0.1, 0, 0, room24),             # no context before the piece: worst case, the room
             (0, 0.7, 0, 0, room24),             # a ratio of 0.7 is never trusted
             (0, 0.02, 1, 0, None),              # 1 145 728 free / max(0.05, 0.03), under the memory bound of 2^30 / 28
             (0, 1.0, 0, 0, 1 << 22)]            # the override
    got = run(exe, tmp_path, "".join("walk " + " ".join(str(x) for x in c) + "\n" for c in filled_cases()))
    firsts, fresh = [], True
    for ln in got:
        if ln[0] == "walked":
            fresh = True
        elif fresh:
            p = dict(zip(PIECE_KEYS, ln[1:]))
            firsts.append((int(p["have_ratio"]), float(p["dup_ratio"]), int(p["trusted"]), int(p["histo_request"]), int(p["end"]) - int(p["pos"])))
            fresh = False
    assert len(firsts) == len(wants)
    for f, w in zip(firsts, wants):
        assert f[:4] == w[:4] and (w[4] is None or f[4] == w[4]), (f, w)
    assert 22_914_559 <= firsts[7][4] <= 22_914_560
    # the ratio a piece measured is the next one's: 80 000 new keys per million bases, rounded down to whole keys
    after = [ln for ln in got if ln[0] == "piece" and ln[1] == str(room24)]
    assert after and float(after[0][10]) == 766_632 / 9_582_912 and after[0][9] == "0" and after[0][8] == "1"


def test_piece_window_by_hand(exe, tmp_path):
    cases = [((0, 100, 30, 0), (0, 100, 0)), ((10, 100, 30, 9), (0, 100, 10)), ((30, 100, 30, 0), (0, 100, 30)), ((46, 100, 30, 0), (16, 84, 30)), ((47, 100, 30, 0), (16, 84, 31)),
             ((47, 100, 30, 1), (15, 85, 32)), ((47, 100, 30, 15), (17, 83, 30)), ((40, 100, 30, 15), (1, 99, 39)), ((35, 100, 30, 9), (0, 100, 35)),
             ((12_582_912, 21_004_295, 36, 9), (12_582_871, 8_421_424, 41)), ((1 << 34, (1 << 34) + 5, 63, 3), ((1 << 34) - 67, 72, 67))]
    got = run(exe, tmp_path, "".join("window %d %d %d %d\n" % c for c, _ in cases))
    assert got == [["window"] + [str(x) for x in w] for _, w in cases]
    for (pos, end, halo, mis), w in cases:
        assert window(pos, end, halo, mis) == w


# ---- growth ---------------------------------------------------------------------------------------------------------------------------
def test_growth_targets_by_hand(exe, tmp_path):
    S = 1 << 20
    grow = [((S // 2, 500, 20, 62), (0, 21)), ((S // 2 + 1, 500, 20, 62), (1, 22)), ((S, 500, 20, 62), (1, 22)), ((S + 1, 500, 20, 62), (1, 23)), ((S // 4, 500, 20, 62), (0, 21)),
            ((S // 4 + 1, 500, 20, 62), (0, 21)), ((3 * S // 4 + 1, 750, 20, 62), (1, 22)), ((3 * S // 4, 750, 20, 62), (0, 21)), ((1 << 40, 500, 20, 22), (1, 22)),
            ((1 << 40, 500, 22, 22), (0, 23)), ((1 << 40, 500, 20, 21), (1, 21))]
    cap = [((0, 3 * S // 4, 20, 62), 20), ((0, 3 * S // 4 + 1, 20, 62), 21), ((S // 4, S // 2, 20, 62), 20), ((S // 4 + 1, S // 2, 20, 62), 21), ((0, 3 * S // 2, 20, 62), 21),
           ((1, 3 * S // 2, 20, 62), 22), ((0, 1 << 40, 20, 24), 24), ((0, 1 << 40, 24, 24), 24), ((0, 0, 20, 62), 20)]
    load = [((0, 0, 3 * S // 4, S), 0), ((0, 1, 3 * S // 4, S), 1), ((S // 4, S // 4, S // 4, S), 0), ((S // 4, S // 4 + 1, S // 4, S), 1), ((1, 0, 3 * S // 4, S), 1)]
    text = "".join("grow %d %d %d %d\n" % c for c, _ in grow) + "".join("cap %d %d %d %d\n" % c for c, _ in cap) + "".join("load %d %d %d %d\n" % c for c, _ in load)
    got = run(exe, tmp_path, text)
    assert got == [["grow", str(a), str(b)] for _, (a, b) in grow] + [["cap", str(w)] for _, w in cap] + [["load", str(w)] for _, w in load]
    # the rules the hand cases were worked out from
    for (d, pm, s, B), (full, ns) in grow:
        assert full == int(d > pm / 1000 * (1 << s) and s < B)
        t = s + 1
        while d > 0.5 * pm / 1000 * (1 << t) and t < B:
            t += 1
        assert t == ns
    for (d, up, s, B), ns in cap:
        t = s
        while d + up > 0.75 * (1 << t) and t < B:
            t += 1
        assert t == ns
