// count_plan.hpp -- everything the counting path computes on the host: the geometry of the two list levels of a partitioned piece
// (count_part.hip), the same for the exchange between GPUs, the sizes of a piece's buffers and launches, how a call is cut into
// pieces (table.hip: count_device) and when the table grows.  Plain C++: no HIP call, no getenv -- what the environment switches
// say comes in as a CountOptions, filled by CountOptions::from_env on the HIP side.  Every rank of a multi-GPU run must derive
// bit-identical geometry from these functions.  tools/count_plan_check.cpp builds the header stand-alone under sanitizers
// (tests/test_count_plan_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace jk {

constexpr uint32_t MAX_SHARDS = 8;   // the GPUs of one node

constexpr int PT_THREADS = 1024;
constexpr int PT_GROUP = 16;
constexpr int PT_TILE = PT_THREADS * PT_GROUP;   // 16384 records per block iteration
constexpr int PT_MAXBUCKETS = 2048;              // p1, p2 <= 11
constexpr int RG_MAXBITS = 12;                   // region = 4096 slots: 48 KB of LDS in region_insert_kernel, three workgroups per CU (8192 for the largest tables)
constexpr uint64_t PIECE_MIN = 8u << 20;         // smaller pieces: the direct kernel is already latency-hidden
constexpr int BIG_LDS = 160 * 1024;              // the whole LDS of a CU
constexpr int P2F_LINE = 16;                     // records per 128-byte line
constexpr int LDS_HBINS = 1024;                  // histogram bins kept in LDS by region_insert_kernel (higher multiplicities are rare: global atomics)
constexpr int LI_MAXSL = 64;                     // slices per region an owner reads (region_insert_kernel<., XCHG>)
constexpr uint64_t PIECE_MAX = 1ull << 33;       // (positions are 64-bit throughout; slice counters are 32-bit but per slice)

// geometry of the two list levels of the partitioned counting path (count_part.hip); its kernels take it by value
struct PartGeom {
    int p1, p2, rbits;       // p1 + p2 + rbits == s
    int recbits;             // 2k - p1: bits kept in a record (<= 64: 8-byte records; more, for keys of more than 74 bits: 16-byte records)
    uint32_t nblk1;          // slices per level-1 list: the part1 blocks b, b + nblk1, b + 2 nblk1, ... append to slice b % nblk1 of every list
    uint32_t grid1;          // part1 blocks
    uint32_t nblk2;          // part2 blocks per level-1 bucket: every one owns a slice of each of the bucket's region lists
    uint32_t cap1, cap2;     // slice capacities (records)
};

// what the environment switches say.  The pure functions below take it and never call getenv; from_env (count_part.hip) reads
// the per-call switches each time it is called -- tests flip them in-process between calls -- and the two tuning experiments
// once per process.
struct CountOptions {
    bool direct = false;                 // JASPER_COUNT_DIRECT: no partitioned pieces
    bool no_rec16 = false;               // JASPER_COUNT_NO_REC16: none with 16-byte records
    bool no_wide = false;                // JASPER_COUNT_NO_WIDE: none into a wide table
    int ngrp = 0, nblk2 = 0;             // JASPER_EXPERIMENT_NGRP, _NBLK2 (tuning experiments only; 0: not set)
    bool xchg_rb12 = false, xchg_rb13 = false;      // JASPER_EXPERIMENT_XCHG_RB12 / _RB13: force the owners' region size
    int xchg_max_lists = PT_MAXBUCKETS;  // JASPER_XCHG_TEST_MAXLISTS (tests: force the owner's extra pass on small tables)
    bool piece_set = false;              // JASPER_EXPERIMENT_PIECE (tuning experiments only): every piece this long, no room made up front
    uint64_t piece = 0;
    static CountOptions from_env();      // (defined in count_part.hip)
};

struct TableShape { int k, B, s; bool ext; uint64_t nslots; };      // B = 2k, nslots = 2^s; ext: a wide table (second word per slot)

inline uint32_t list_cap(double avg) { return (uint32_t)std::min<double>(4.0e9, avg * 1.25 + 8.0 * std::sqrt(avg) + 64.0); }

// can this piece take the partitioned path, and with which geometry?
inline bool partition_geometry(const TableShape &t, uint64_t piece_bases, const CountOptions &opt, PartGeom &G) {
    if (opt.direct) return false;
    if (piece_bases < PIECE_MIN) return false;
    const int B = t.B, s = t.s;
    // 8-byte records hold the hash below the p1 <= 10 bucket bits: keys of up to 74 bits (k <= 37).  Longer keys travel as
    // 16-byte records (part1w_kernel, part2f_kernel<., ., ., Rec16>, region_insert_kernel<., ., Rec16>): half the records per LDS round.
    const bool rec16 = B > 74;
    if (rec16 && opt.no_rec16) return false;
    if (t.ext && !rec16) return false;                    // (a tiny table for short keys: its images would need the second word for 8-byte records)
    if (t.ext && opt.no_wide) return false;
    const int need_p1 = rec16 ? std::min(10, s - 12) : (B > 64 ? B - 64 : 0);
    // regions of 2^12 slots (three region_insert workgroups per CU); 2^13 only where the two list levels cannot split finer
    int p1 = 0, p2 = 0;
    bool ok = false;
    // (first choice: at most 512 lists per bucket, which part2f_kernel writes in whole lines)
    // (a wide table's image is 20 bytes per slot: regions of 2^11)
    const int rg0 = t.ext ? RG_MAXBITS - 1 : RG_MAXBITS;
    for (int maxp2 = 9; maxp2 <= (rec16 ? 9 : 11) && !ok; maxp2 += 2)
    for (int rg = rg0; rg <= rg0 + 1 && !ok; ++rg) {
        p1 = std::max(need_p1, (s - rg + 1) / 2);
        if (p1 < 1) p1 = 1;
        if (p1 > 10 || p1 > s - 8) continue;              // (a table too small to be worth it)
        p2 = s - rg - p1;
        if (p2 < 0) p2 = 0;
        ok = p2 <= maxp2;
    }
    if (!ok) return false;
    G.p1 = p1; G.p2 = p2; G.rbits = s - p1 - p2; G.recbits = B - p1;
    // one 1024-thread block (159 KB of LDS) per CU; the blocks of an XCD (b, b + 8, ...) share their slices (part1_kernel)
    const uint64_t tile1 = (uint64_t)PT_TILE;
    const uint64_t ntiles = (piece_bases + tile1 - 1) / tile1;
    uint64_t grid1 = piece_bases / ((uint64_t)(1u << p1) * 512);
    grid1 = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(grid1, ntiles), 256));
    // (measured, 47 Mb workload, round 4's kernel with the fill counts slice-major: 2 to 16 slices per list 4.0-4.1 ms, 32 slices 4.2,
    //  ONE slice 5.3 -- 256 blocks adding to each count; with the counts bucket-major a wave's 64 atomics were 8 x nblk1 requests
    //  to the memory side, which alone took 4.4 ms at 2 slices and more at 8.  8 slices: part2f's 16 waves find slices of their own)
    const uint64_t nblk1 = std::min<uint64_t>(grid1, opt.ngrp > 0 ? (uint64_t)opt.ngrp : 8);
    G.grid1 = (uint32_t)grid1;
    G.nblk1 = (uint32_t)nblk1;
    // (a slice takes the tiles of ceil(grid1 / nblk1) blocks of ceil(ntiles / grid1) tiles each)
    const uint64_t tiles_per_slice = ((grid1 + nblk1 - 1) / nblk1) * ((ntiles + grid1 - 1) / grid1);
    // (a level-1 slice holds half a million records and more: 10 % above the BASES that can fall into it -- records are ~3/4 of the
    //  bases -- is slack for a bucket with a very frequent k-mer; what does not fit is deferred.  Device memory that has been used
    //  before is cleared when it is allocated again, ~28 ms per GB on some boxes: every GB of slack shows in a first call.)
    const double avg1 = (double)std::min<uint64_t>(piece_bases, tiles_per_slice * tile1) / (double)(1u << p1);
    G.cap1 = avg1 >= 65536.0 ? (uint32_t)std::min<double>(4.0e9, avg1 * 1.10 + 8.0 * std::sqrt(avg1) + 64.0) : list_cap(avg1);
    // one slice per region list: part2 runs one 1024-thread block per CU, and 2^p1 >= 256 buckets already fill the chip;
    // region_insert_kernel then reads a region's records as one contiguous list
    G.nblk2 = p2 ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nblk1, opt.nblk2 > 0 ? opt.nblk2 : ((1u << p1) >= 256 ? 1 : 8))) : 1;
    G.cap2 = p2 ? (list_cap((double)piece_bases / ((double)(1ull << (p1 + p2)) * (double)G.nblk2)) + 15u) & ~15u : 0;      // whole 128-byte lines (part2f_kernel)
    return true;
}

// the direct kernel or the list passes?  The partitioned path streams the whole table once per piece: worth it only for pieces
// that are large relative to the table (host-staged 64 MiB pieces stay on the direct kernel and are PCIe-bound anyway).
// Break-even measured on MI355X: direct ~18 Gk-mers/s; partitioned ~55 Gk-mers/s for the two list passes plus one
// streaming pass over the table (32 B/slot, 16 B/slot when the table is still lazily cleared)
inline bool piece_worth_partitioning(uint64_t len, uint64_t nslots, bool slots_dirty) { return len >= (slots_dirty ? nslots / 6 : nslots / 4); }

// which instance of the second pass: every level-1 bucket -> nown x 2^p2 lists (nown = 1: one GPU; by_owner: laid out owner-major,
// part2_kernel).  The whole-line kernel takes what it can: at most 512 lists per bucket and slices of whole lines; 16-byte
// records have no other (none: "count: no list geometry for 16-byte records").  old_p2: JASPER_EXPERIMENT_OLDP2, the general kernel
// where the whole-line one would do.
enum class Part2Kind { none, rec16_lines, owner_lines, lines128, lines512, general_owner, general };
inline Part2Kind part2_instance(const PartGeom &G, uint32_t nown, bool by_owner, bool old_p2) {
    const uint64_t nlists = (uint64_t)nown << G.p2;            // per bucket
    const bool rec16 = G.recbits > 64;
    const bool lines = nlists <= 512 && G.cap2 % P2F_LINE == 0;
    if (rec16) return lines ? Part2Kind::rec16_lines : Part2Kind::none;
    if (lines && !old_p2) return by_owner ? Part2Kind::owner_lines : nlists <= 128 ? Part2Kind::lines128 : Part2Kind::lines512;
    return by_owner ? Part2Kind::general_owner : Part2Kind::general;
}

// region_insert's launch: the LDS image of a region of 2^rbits slots and the number of workgroups
struct RegionLaunch { size_t lds; uint32_t blocks; };
inline RegionLaunch region_insert_launch(int rbits, uint32_t nregions, bool ext, bool fresh, bool histo, bool xchg) {
    const size_t R = (size_t)1 << rbits;
    // (a wide table's image: tag, second word and count per slot, no histogram bins)
    const size_t lds = xchg ? R * 16 + LDS_HBINS * 4 + (LI_MAXSL + 1) * 4 : ext ? R * (fresh ? 20 : 24) : R * (fresh ? 12 : 16) + (histo ? LDS_HBINS * 4 : 0);
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(4, BIG_LDS / lds));
    return {lds, std::max<uint32_t>(1, std::min<uint32_t>(nregions, 256 * per_cu * 4))};
}

// the buffers of a partitioned piece of len bases (launch_count_partitioned)
struct PieceBuffers {
    uint32_t nb1, nregions;      // level-1 buckets, regions
    size_t n_cnt1, n_cnt2;       // fill counts of the two levels (one level: the counts once more, bucket-major)
    size_t rec_bytes;            // 8 or 16
    uint64_t deferred_cap;       // (24 bytes each; a piece that needs more abandons itself: part_decide_kernel)
};
inline PieceBuffers piece_buffers(const PartGeom &G, uint64_t len) {
    PieceBuffers b;
    b.nb1 = 1u << G.p1;
    b.nregions = 1u << (G.p1 + G.p2);
    b.n_cnt1 = (size_t)b.nb1 * G.nblk1;
    b.n_cnt2 = G.p2 ? (size_t)b.nregions * G.nblk2 : b.n_cnt1;
    b.rec_bytes = G.recbits > 64 ? 16 : 8;
    b.deferred_cap = std::max<uint64_t>(1u << 16, len / 48);
    return b;
}
// A table that is logically empty is not read: the images start from zeros and every slot is written (a lazily cleared table
// is never zeroed in HBM).  Its LDS image counts in 32 bits -- a piece below 2^32 bases cannot overflow them.
inline bool piece_fresh32(bool empty_tbl, uint64_t len) { return empty_tbl && len < (1ull << 32); }

// ---- the exchange between GPUs ------------------------------------------------------------------------------------------------------
// All ranks must derive the same geometry: from the shard geometry (one for all owners), the number of owners, piece_max =
// the longest piece any rank scans in this round, and records_max = the most records any rank's scan produced (0: not known,
// piece_max stands in).  The slack of the send lists is what travels, so they are sized from the records actually there, not
// with the 1.25x of the local lists: mean + 6 sigma, where a list's fill is a sum over the distinct keys hashed into it of
// their multiplicities in this sender's reads -- variance = mean x (1 + multiplicity).  The multiplicity is estimated from the
// table the caller sized for the keys (about a third full): records / (keys all shards were sized for).  A list that still
// overflows (a k-mer far more frequent than the rest, or a table sized far too large) spends the deferred list, as everywhere.
inline uint32_t xchg_cap(double avg, double mult) { return (uint32_t)std::min<double>(4.0e9, avg + 6.0 * std::sqrt(avg * (1.0 + mult)) + 16.0); }
// G: what the senders and the wire use (G.p2 = the second-level bits the SENDER resolves); p2b: second-level bits left to the
// owner -- a bucket can be split 2048 ways in one pass, and the senders also split by owner, so for very large shards (2^32
// slots on 8 GPUs) the owner runs one more split pass over what it received (part2_kernel<false, MIN>) before its insert.
// (returns p2b, or -1: no geometry)
inline int xchg_geometry(const TableShape &t, uint64_t piece_max, uint64_t records_max, uint32_t nown, const CountOptions &opt, PartGeom &G) {
    if (nown < 2 || nown > MAX_SHARDS) return -1;
    // (a feed's last batch may be small: the lists are then laid out as for the smallest piece the passes are tuned for)
    piece_max = std::max<uint64_t>(piece_max, PIECE_MIN);
    if (!partition_geometry(t, piece_max, opt, G)) return -1;
    if (G.recbits > 64) return -1;                        // (keys of more than 74 bits: per-GPU tables and the entry exchange instead)
    // the senders split by (owner, second-level bits): more than 512 lists per bucket would leave the whole-line kernel, so the
    // owners take regions of 8192 slots instead of 4096 where that is what it takes -- for up to four owners, whose lists travel
    // deduplicated (dist.dedupe_pays).  Beyond that the lists travel as they are, and an owner inserting 10^9 raw records into
    // 8192-slot regions (one workgroup per CU) takes 8.6 ms against 5.7 into 4096-slot ones, which the general split kernel's
    // 5.7 ms against 4.6 does not eat up (role-play at 8 ranks, profiles/round5/exchange_roleplay_model.txt: 15.7 against 17.3 ms
    // of kernels per rank).  JASPER_EXPERIMENT_XCHG_RB12 / _RB13 force one or the other.
    const bool rb13 = opt.xchg_rb13 ? true : opt.xchg_rb12 ? false : nown <= 4;
    if (((uint64_t)nown << G.p2) > 512 && ((uint64_t)nown << (G.p2 - 1)) <= 512 && G.p2 > 0 && G.rbits == RG_MAXBITS && rb13) { --G.p2; ++G.rbits; }
    int p2b = 0;
    while (((uint64_t)nown << (G.p2 - p2b)) > (uint64_t)opt.xchg_max_lists && p2b < G.p2) ++p2b;
    if (((uint64_t)nown << (G.p2 - p2b)) > (uint64_t)PT_MAXBUCKETS) return -1;
    G.p2 -= p2b;
    const uint32_t nb1 = 1u << G.p1;
    G.nblk2 = nb1 >= 256 ? 1u : std::min<uint32_t>(G.nblk1, 8u);
    if (nown * G.nblk2 > (uint32_t)LI_MAXSL) return -1;
    const double lists = (double)nb1 * (double)((uint64_t)nown << G.p2) * (double)G.nblk2;
    if (records_max) {
        const double rec = (double)std::min(records_max, piece_max);
        const double keys = std::max(1.0, std::min(rec, 0.35 * (double)t.nslots * (double)nown));
        G.cap2 = xchg_cap(rec / lists, rec / keys);
    } else G.cap2 = list_cap((double)piece_max / lists);
    G.cap2 = (G.cap2 + 15u) & ~15u;                       // whole 128-byte lines (part2f_kernel<., ., OWN>)
    return p2b;
}
// deferred entries (24 B) a rank may produce in a round of the exchange, and an owner's insert of its own
inline uint64_t xchg_defer_cap(uint64_t piece_max) { return std::max<uint64_t>(1u << 16, piece_max / 16); }
// what xchg_plan tells the caller
inline void xchg_plan_words(const PartGeom &G, int p2b, uint64_t piece_max, uint64_t out[8]) {
    const uint64_t lists_per_owner = (uint64_t)1 << (G.p1 + G.p2);
    out[0] = lists_per_owner * G.nblk2 * G.cap2;               // records (8 B) per owner block
    out[1] = lists_per_owner * G.nblk2;                        // slice counts (4 B) per owner block
    out[2] = xchg_defer_cap(piece_max);                        // deferred entries (24 B) a rank may produce
    out[3] = (uint64_t)G.p1; out[4] = (uint64_t)G.p2 | ((uint64_t)p2b << 8); out[5] = (uint64_t)G.rbits; out[6] = G.nblk2; out[7] = G.cap2;
}
// The owner's side (xchg_insert).  G: the wire's geometry (cap2 = the slices as they arrived: packed by the caller after
// xchg_dedupe, or the senders' own).  GI: what region_insert sees, all second-level bits resolved.  G2, for p2b > 0: the senders
// resolved only G.p2 of the second-level bits, so one more split pass runs over what arrived.  Its buckets are the received lists
// (2^(p1 + G.p2) of them, nown * nblk2 slices each), its record bits the ones below those lists' bits.
struct OwnerSplit { PartGeom G2, GI; uint32_t nregions; };
inline OwnerSplit xchg_owner_split(const PartGeom &G, int p2b, uint32_t nown, uint64_t records_max) {
    OwnerSplit o;
    o.nregions = 1u << (G.p1 + G.p2 + p2b);
    o.GI = G;
    o.GI.p2 = G.p2 + p2b;
    o.G2 = G;
    o.G2.p1 = G.p1 + G.p2; o.G2.p2 = p2b; o.G2.recbits = G.recbits - G.p2;
    o.G2.nblk1 = nown * G.nblk2; o.G2.cap1 = G.cap2; o.G2.nblk2 = 1;
    o.G2.cap2 = list_cap((double)std::max<uint64_t>(records_max, 1) / (double)o.nregions);
    return o;
}

// ---- a call's pieces (count_device) -------------------------------------------------------------------------------------------------
// A piece starts `halo` = k-1 bases early, rounded down so that (text + start) is 16-byte aligned -- the kernels keep their 16-byte
// vector loads; emit_from keeps every window counted exactly once.  misalign = the text's address & 15.
struct PieceWindow { uint64_t start, len, emit_from; };
inline PieceWindow piece_window(uint64_t pos, uint64_t end, uint64_t halo, uint64_t misalign) {
    uint64_t start = pos >= halo ? pos - halo : 0;
    const uint64_t a = (start + misalign) & 15;
    start = start >= a ? start - a : 0;
    return {start, end - start, pos - start};
}

struct Piece {
    uint64_t start, end;         // text [start, end): context from start, new bases from start + emit_from
    uint64_t emit_from;
    uint64_t expect_new;         // new keys the piece is expected to bring (worst case where the ratio is not trusted)
    bool needs_room;             // ... more than fit under 3/4 full: the table grows up front
    bool histo_request;          // one piece, whole input, empty table: the multiplicity histogram can be fused into it
};

// How a call is cut into pieces.  Bases already in HBM are processed in launches that keep the table under 3/4 full in the worst
// case, so that the load factor is re-checked (and the table grown) between launches.
struct PiecePlan {
    double dup_ratio = 1.0;      // new distinct keys per k-mer of the last piece (sizes the next piece); carried from call to call
    bool have_ratio = false;     // this call's ratio comes from the caller's size hint
    bool started_empty = false;

    // Before anything has been measured, the caller's size hint plays the role of `jellyfish count -s`: the expected
    // number of distinct k-mers of this input.  hint / bases is then the expected share of new keys per k-mer; it is
    // only trusted for sizing the pieces (x1.5 below) -- an input that is less repetitive than promised still ends up
    // in the spill / deferred lists and a grown table, or in a clean error, never in wrong counts.
    void begin(uint64_t size_hint, uint64_t n, uint64_t distinct, uint64_t occurrences) {
        have_ratio = false;
        started_empty = distinct == 0 && occurrences == 0;
        if (size_hint > 0 && n > (1u << 24) && started_empty) {
            dup_ratio = std::min(1.0, (double)size_hint / (double)n);
            have_ratio = dup_ratio < 0.6;
        }
    }
    // after the first piece the measured share of NEW keys per k-mer (x1.5 safety) replaces the worst case "every base
    // a new key"; the spill list / deferred list / growth still catch a piece that turns out less repetitive
    bool trusted(uint64_t pos) const { return (pos > 0 || have_ratio) && dup_ratio < 0.6; }

    // the piece that begins at pos of n bases (bases before first_new are context only); distinct: the table's keys at the last
    // check; mem_have: device memory the lists may take (0: not known) -- they need ~20 bytes of workspace per base
    Piece next(uint64_t pos, uint64_t n, uint64_t first_new, uint64_t distinct, uint64_t nslots, uint64_t mem_have, uint64_t halo, uint64_t misalign,
               const CountOptions &opt) const {
        // a launch may add at most as many new keys as keep the table under 3/4 full in the worst case (every
        // base a new k-mer)
        const uint64_t room = (uint64_t)(0.75 * (double)nslots) > distinct ? (uint64_t)(0.75 * (double)nslots) - distinct : 0;
        uint64_t piece = std::max<uint64_t>(room, 1u << 20);
        if (trusted(pos)) piece = std::max<uint64_t>(piece, (uint64_t)((double)room / std::max(0.05, 1.5 * dup_ratio)));
        if (mem_have) piece = std::min<uint64_t>(piece, std::max<uint64_t>(mem_have / 28, 1u << 20));
        piece = std::min<uint64_t>(piece, PIECE_MAX);
        // do not leave a small tail for a separate launch (the 1.5x safety factor covers a quarter more)
        if (trusted(pos) && n - pos <= piece + piece / 4 && n - pos <= PIECE_MAX) piece = n - pos;
        // the caller's own promise (size hint = expected distinct k-mers of this input) fits the free room: one piece
        if (have_ratio && pos == 0 && (double)n * dup_ratio <= (double)room && n <= PIECE_MAX && (!mem_have || n <= mem_have / 28)) piece = n;
        if (opt.piece_set) piece = opt.piece;
        Piece p;
        // room up front for the new keys this piece is expected to bring (worst case for the first piece)
        const uint64_t todo = std::min<uint64_t>(piece, n - pos);
        // (the share of new keys only falls as coverage accumulates, so the last piece's ratio is already an upper
        // estimate; spill list, deferred list and growth after the piece remain the safety net)
        p.expect_new = trusted(pos) ? (uint64_t)((double)todo * std::min(1.0, dup_ratio)) : todo;
        p.needs_room = p.expect_new > room && !opt.piece_set;
        p.end = std::min<uint64_t>(n, pos + piece);
        const PieceWindow w = piece_window(pos, p.end, halo, misalign);
        p.start = w.start;
        p.emit_from = w.emit_from;
        p.histo_request = started_empty && pos == 0 && first_new == 0 && p.end == n && distinct == 0;
        return p;
    }
    void observe(uint64_t distinct_delta, uint64_t occurrence_delta) {
        if (occurrence_delta) dup_ratio = (double)distinct_delta / (double)occurrence_delta;
    }
    // The size hint promised a more repetitive input than this one: worst-case piece sizes from here on
    void restart_worst_case() { have_ratio = false; dup_ratio = 1.0; }
};

// ---- growth -------------------------------------------------------------------------------------------------------------------------
// after a batch of insertions: past the load limit?  and the size to grow to: at most half the limit
inline bool table_too_full(uint64_t distinct, double grow_at, uint64_t nslots, int s, int B) { return (double)distinct > grow_at * (double)nslots && s < B; }
inline int grow_target(uint64_t distinct, double grow_at, int s, int B) {
    int ns = s + 1;
    while ((double)distinct > 0.5 * grow_at * (double)(1ull << ns) && ns < B) ++ns;
    return ns;
}
// keep the worst case (every upcoming k-mer new) under 3/4 full so probe runs stay far below MAXPROBE
inline int capacity_target(uint64_t distinct, uint64_t upcoming_kmers, int s, int B) {
    int ns = s;
    while ((double)(distinct + upcoming_kmers) > 0.75 * (double)(1ull << ns) && ns < B) ++ns;
    return ns;
}
// count_host's streaming loop: could the worst case (all of the pending and the next piece's bases new keys) pass 3/4?
inline bool worst_case_passes_load(uint64_t distinct, uint64_t pending, uint64_t piece, uint64_t nslots) {
    return (double)(distinct + pending + piece) > 0.75 * (double)nslots;
}

}  // namespace jk
