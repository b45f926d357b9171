// count_plan_check.cpp -- jasper_amd/csrc/count_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_count_plan_host.py).  No HIP, no GPU, no environment: the switches are numbers of the case file.
//
//   count_plan_check FILE
//
// FILE holds tokens separated by blanks: commands, each a word and its numbers; the program prints one line per command (a walk:
// one per piece and a closing one) and `ok` at the end.  OPT = direct no_rec16 no_wide ngrp nblk2 rb12 rb13 maxlists (0: none).
//
//   geom k s ext piece OPT                 -> "geom 0" (refused) or "geom 1 p1 p2 rbits recbits nblk1 grid1 nblk2 cap1 cap2"
//   xchg k s piece_max records_max nown OPT
//                                          -> "xchg -1" or "xchg p2b p1 p2 rbits recbits nblk1 grid1 nblk2 cap1 cap2 | w0 .. w7 |
//                                             nregions G2.p1 G2.p2 G2.recbits G2.nblk1 G2.cap1 G2.nblk2 G2.cap2 GI.p1 GI.p2 GI.rbits GI.recbits"
//   bufs p1 p2 recbits nblk1 nblk2 len     -> "bufs nb1 nregions n_cnt1 n_cnt2 rec_bytes deferred_cap"
//   fresh32 empty len                      -> "fresh32 0/1"
//   part2 recbits p2 cap2 nown by_owner old_p2   -> "part2 kind" (none rec16_lines owner_lines lines128 lines512 general_owner general)
//   region rbits nregions ext fresh histo xchg   -> "region lds blocks"
//   worth len nslots dirty                 -> "worth 0/1"
//   window pos end halo misalign           -> "window start len emit_from"
//   grow distinct grow_at_permille s B     -> "grow too_full ns"
//   cap distinct upcoming s B              -> "cap ns"
//   load distinct pending piece nslots     -> "load 0/1"
//   walk k s n first_new misalign hint mem_have piece_override ratio_ppm restart_at distinct0 occ0 carried_ppm
//        a call of n bases into a table of 2^s slots that holds distinct0 keys and occ0 occurrences, its dup_ratio carried from
//        the call before carried_ppm / 10^6; piece_override 0: none; every piece brings ratio_ppm new keys per million new
//        bases; restart_at: the piece (by number) after which the size-hint restart happens, -1: none
//                                          -> per piece "piece pos start end emit_from expect_new needs_room histo_request trusted
//                                             have_ratio dup_ratio distinct s", then "walked pieces"
#include "count_plan.hpp"

#include <cstdio>
#include <fstream>
#include <string>

using namespace jk;

static bool read_opt(std::istream &in, CountOptions &o) {
    int direct = 0, no_rec16 = 0, no_wide = 0, rb12 = 0, rb13 = 0, maxlists = 0;
    in >> direct >> no_rec16 >> no_wide >> o.ngrp >> o.nblk2 >> rb12 >> rb13 >> maxlists;
    o.direct = direct != 0; o.no_rec16 = no_rec16 != 0; o.no_wide = no_wide != 0; o.xchg_rb12 = rb12 != 0; o.xchg_rb13 = rb13 != 0;
    if (maxlists) o.xchg_max_lists = std::max(2, maxlists);
    return (bool)in;
}
static TableShape shape_of(int k, int s, bool ext) { return {k, 2 * k, s, ext, 1ull << s}; }
static void print_geom(const PartGeom &G) { std::printf(" %d %d %d %d %u %u %u %u %u", G.p1, G.p2, G.rbits, G.recbits, G.nblk1, G.grid1, G.nblk2, G.cap1, G.cap2); }

static int do_geom(std::istream &in) {
    int k = 0, s = 0, ext = 0;
    uint64_t piece = 0;
    CountOptions o;
    in >> k >> s >> ext >> piece;
    if (!read_opt(in, o)) return 2;
    PartGeom G{};
    const bool ok = partition_geometry(shape_of(k, s, ext != 0), piece, o, G);
    std::printf("geom %d", (int)ok);
    if (ok) print_geom(G);
    std::printf("\n");
    return 0;
}

static int do_xchg(std::istream &in) {
    int k = 0, s = 0;
    uint64_t piece_max = 0, records_max = 0;
    uint32_t nown = 0;
    CountOptions o;
    in >> k >> s >> piece_max >> records_max >> nown;
    if (!read_opt(in, o)) return 2;
    PartGeom G{};
    const int p2b = xchg_geometry(shape_of(k, s, false), piece_max, records_max, nown, o, G);
    std::printf("xchg %d", p2b);
    if (p2b >= 0) {
        print_geom(G);
        uint64_t w[8];
        xchg_plan_words(G, p2b, piece_max, w);
        std::printf(" |");
        for (uint64_t x : w) std::printf(" %llu", (unsigned long long)x);
        const OwnerSplit S = xchg_owner_split(G, p2b, nown, records_max);
        std::printf(" | %u %d %d %d %u %u %u %u %d %d %d %d", S.nregions, S.G2.p1, S.G2.p2, S.G2.recbits, S.G2.nblk1, S.G2.cap1, S.G2.nblk2, S.G2.cap2, S.GI.p1, S.GI.p2, S.GI.rbits,
                    S.GI.recbits);
    }
    std::printf("\n");
    return 0;
}

static int do_bufs(std::istream &in) {
    PartGeom G{};
    uint64_t len = 0;
    in >> G.p1 >> G.p2 >> G.recbits >> G.nblk1 >> G.nblk2 >> len;
    if (!in) return 2;
    const PieceBuffers b = piece_buffers(G, len);
    std::printf("bufs %u %u %zu %zu %zu %llu\n", b.nb1, b.nregions, b.n_cnt1, b.n_cnt2, b.rec_bytes, (unsigned long long)b.deferred_cap);
    return 0;
}

static int do_part2(std::istream &in) {
    PartGeom G{};
    uint32_t nown = 0;
    int by_owner = 0, old_p2 = 0;
    in >> G.recbits >> G.p2 >> G.cap2 >> nown >> by_owner >> old_p2;
    if (!in) return 2;
    static const char *const names[] = {"none", "rec16_lines", "owner_lines", "lines128", "lines512", "general_owner", "general"};
    std::printf("part2 %s\n", names[(int)part2_instance(G, nown, by_owner != 0, old_p2 != 0)]);
    return 0;
}

static int do_walk(std::istream &in) {
    int k = 0, s = 0, restart_at = -1;
    uint64_t n = 0, first_new = 0, misalign = 0, hint = 0, mem_have = 0, override = 0, ratio_ppm = 0, distinct0 = 0, occ0 = 0, carried_ppm = 0;
    in >> k >> s >> n >> first_new >> misalign >> hint >> mem_have >> override >> ratio_ppm >> restart_at >> distinct0 >> occ0 >> carried_ppm;
    if (!in) return 2;
    CountOptions o;
    if (override) { o.piece_set = true; o.piece = override; }
    const int B = 2 * k;
    const double grow_at = 0.5;
    PiecePlan P;
    P.dup_ratio = (double)carried_ppm / 1000000.0;
    uint64_t distinct = distinct0, occ = occ0, pos = std::min(first_new, n);
    P.begin(hint, n, distinct, occ);
    int pieces = 0;
    while (pos < n) {
        if (pieces >= 100000) return 3;
        const Piece p = P.next(pos, n, first_new, distinct, 1ull << s, mem_have, (uint64_t)(k - 1), misalign, o);
        std::printf("piece %llu %llu %llu %llu %llu %d %d %d %d %.17g %llu %d\n", (unsigned long long)pos, (unsigned long long)p.start, (unsigned long long)p.end,
                    (unsigned long long)p.emit_from, (unsigned long long)p.expect_new, (int)p.needs_room, (int)p.histo_request, (int)P.trusted(pos), (int)P.have_ratio, P.dup_ratio,
                    (unsigned long long)distinct, s);
        if (p.end <= pos) return 4;
        if (p.needs_room) s = capacity_target(distinct, p.expect_new, s, B);
        if (pieces++ == restart_at) {                 // the piece overflowed the table: cleared, grown by two bits, from the start
            P.restart_worst_case();
            distinct = occ = 0;
            s = std::min(B, s + 2);
            pos = std::min(first_new, n);
            continue;
        }
        const uint64_t occ_d = p.end - pos, dist_d = (uint64_t)((unsigned __int128)occ_d * ratio_ppm / 1000000u);
        distinct += dist_d;
        occ += occ_d;
        if (table_too_full(distinct, grow_at, 1ull << s, s, B)) s = grow_target(distinct, grow_at, s, B);
        P.observe(dist_d, occ_d);
        pos = p.end;
    }
    std::printf("walked %d\n", pieces);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: count_plan_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string cmd;
    while (in >> cmd) {
        int rc = 2;
        if (cmd == "geom") rc = do_geom(in);
        else if (cmd == "xchg") rc = do_xchg(in);
        else if (cmd == "bufs") rc = do_bufs(in);
        else if (cmd == "part2") rc = do_part2(in);
        else if (cmd == "walk") rc = do_walk(in);
        else if (cmd == "fresh32") {
            int empty = 0;
            uint64_t len = 0;
            in >> empty >> len;
            std::printf("fresh32 %d\n", (int)piece_fresh32(empty != 0, len));
            rc = in ? 0 : 2;
        } else if (cmd == "region") {
            int rbits = 0, ext = 0, fresh = 0, histo = 0, xchg = 0;
            uint32_t nregions = 0;
            in >> rbits >> nregions >> ext >> fresh >> histo >> xchg;
            const RegionLaunch L = region_insert_launch(rbits, nregions, ext != 0, fresh != 0, histo != 0, xchg != 0);
            std::printf("region %zu %u\n", L.lds, L.blocks);
            rc = in ? 0 : 2;
        } else if (cmd == "worth") {
            uint64_t len = 0, nslots = 0;
            int dirty = 0;
            in >> len >> nslots >> dirty;
            std::printf("worth %d\n", (int)piece_worth_partitioning(len, nslots, dirty != 0));
            rc = in ? 0 : 2;
        } else if (cmd == "window") {
            uint64_t pos = 0, end = 0, halo = 0, misalign = 0;
            in >> pos >> end >> halo >> misalign;
            const PieceWindow w = piece_window(pos, end, halo, misalign);
            std::printf("window %llu %llu %llu\n", (unsigned long long)w.start, (unsigned long long)w.len, (unsigned long long)w.emit_from);
            rc = in ? 0 : 2;
        } else if (cmd == "grow") {
            uint64_t distinct = 0, permille = 0;
            int s = 0, B = 0;
            in >> distinct >> permille >> s >> B;
            const double grow_at = (double)permille / 1000.0;
            std::printf("grow %d %d\n", (int)table_too_full(distinct, grow_at, 1ull << s, s, B), grow_target(distinct, grow_at, s, B));
            rc = in ? 0 : 2;
        } else if (cmd == "cap") {
            uint64_t distinct = 0, upcoming = 0;
            int s = 0, B = 0;
            in >> distinct >> upcoming >> s >> B;
            std::printf("cap %d\n", capacity_target(distinct, upcoming, s, B));
            rc = in ? 0 : 2;
        } else if (cmd == "load") {
            uint64_t distinct = 0, pending = 0, piece = 0, nslots = 0;
            in >> distinct >> pending >> piece >> nslots;
            std::printf("load %d\n", (int)worst_case_passes_load(distinct, pending, piece, nslots));
            rc = in ? 0 : 2;
        }
        if (rc) {
            std::fprintf(stderr, "command %s: %d\n", cmd.c_str(), rc);
            return rc;
        }
    }
    std::printf("ok\n");
    return 0;
}
