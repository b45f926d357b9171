// polish_types.hpp -- the plain structs of the polisher: what the kernels (polish.hip), the host's plan (polish_plan.hpp), the lane
// (polish_host.hip) and the C-ABI (capi.hip) share.  No HIP: a stand-alone program can include it (tools/polish_plan_check.cpp).
#pragma once
#include <cstdint>

namespace jk {

// one fix record (src/jasper.py:218-222 appends [seqname, index, fixed_base, original]); the host turns
// these into CSV rows. 32 bytes.
struct FixRec {
    int64_t index;     // Base_coord (chunk- and pass-relative, as in the reference)
    uint32_t chunk;
    uint32_t seqno;    // order of emission inside (chunk, pass)
    uint8_t pass;
    uint8_t kind;      // 's' substitution, 'i' inserted base(s) removed, 'd' deleted base(s) restored, 'x' path extension
    uint8_t newc;      // 's': new base; 'd': restored base (repeated `rep` times)
    uint8_t oldc;      // 's': old base; 'i': removed base (repeated `rep` times)
    uint32_t rep;      // 'x': length of the original segment
    uint32_t aux_off;  // 'x': offset of  patch ++ original segment  in the aux bytes
    uint32_t aux_len;  // 'x': length of the patch
};
static_assert(sizeof(FixRec) == 32, "FixRec layout");

enum PolishStatus {
    PS_OK = 0,
    PS_GAP_EXHAUSTED = 1,   // text grew beyond its slack
    PS_REC_OVERFLOW = 2,    // more fix records than reserved
    PS_AUX_OVERFLOW = 3,
    PS_BFS_ARENA = 4,       // path-extension search ran out of scratch
    PS_REF_INDEXERROR = 5,  // the reference raises IndexError here (src/jasper.py:221) and exits 1
    PS_STRING_TOO_LONG = 6
};

// position classes written by the dense scan (one byte per window start of a chunk, per pass)
enum PosClass : uint8_t {
    PC_CLEAN = 0,  // valid window, count >= solid_thre, and not (count < count(window k back)/50): the walk does `i += k-1`
    PC_BAD = 1,    // valid window, count < solid_thre
    PC_OTHER = 2   // non-ACGT window, or the k-back test fires / cannot be decided densely: evaluate exactly
};

// One SEGMENT of a chunk record for one pass.  A chunk is cut at "sync points": starts of runs of >= k-1 bad k-mers
// that are preceded by >= 4k clean positions.  Whatever stride phase the reference's walk arrives with, it lands inside
// such a run and handle_bad_kmers() then does the same thing -- so the walk to the right of a sync point does not
// depend on anything to its left except a coordinate shift, and segments can be walked concurrently.
// one text replacement of a segment walk, in the segment's local coordinates AT THE TIME of the edit: local
// [a, a+oldlen) became plen new bytes.  The stitch step replays the list backwards to carry the position classes of
// untouched windows over to the next pass instead of recomputing them.
struct EditRec {
    int64_t a;
    int32_t plen, oldlen;
};

struct SegDev {
    uint8_t *buf;        // gap buffer holding a private copy of the segment's text (local coordinates)
    int64_t cap;
    int64_t len;         // logical length (local)
    int64_t gs, glen;    // gap start / length
    int64_t len0;        // logical length before the pass
    int64_t seg_lo;      // chunk coordinate (at pass start) of local position 0
    int64_t start_i;     // local position where the walk starts (0 for the first segment of a chunk)
    int64_t stop_orig;   // the walk ends when it arrives at an event whose pass-start chunk coordinate is >= this
    int32_t first, last; // first / last segment of its chunk: chunk-start / chunk-end semantics are real there
    // A segment whose left boundary is a CLEAN-ZONE boundary (not a sync point) does not know where the walk arrives: it
    // takes the arrival position its predecessor publishes (chain_in = 1).  Every segment publishes the chunk coordinate
    // (pass-start text) at which it handed over in *arrive: ARRIVE_PENDING until then, ARRIVE_FAIL if it gave up.
    int32_t chain_in;
    int32_t took_shortcut;   // out: the range held no event, the arrival was computed instead of walked
    long long *arrive;   // this segment's slot; the predecessor's is arrive[-1]
    const uint8_t *cls;  // PosClass per window start of the chunk at pass start (chunk coordinates), cls_n entries
    int64_t cls_n;
    FixRec *recs;
    uint32_t rec_cap, nrec;
    uint8_t *aux;
    uint32_t aux_cap, naux;
    EditRec *edits;
    uint32_t edit_cap, nedit;
    uint32_t chunk;
    int32_t status;
    int32_t spec_fail;   // the walk touched text outside what the segment may assume -> redo the chunk unsegmented
    int64_t wrong;       // bad k-mers counted in this segment during this pass
    uint64_t lookups;
    uint64_t ticks;      // wall_clock64() ticks (100 MHz) this segment's walk took -- tuning aid
    uint64_t tk[12];     // of which: [0] skipping good k-mers, [1] finding the bad run, [2] choosing a fix, [3] splicing the text;
                         // [4..10] inside [2]: fix_k_case_sub, fix_insert, fix_del, fixdiploid, fix_same_base_del,
                         // fix_same_base_insertion, base_extension
    // filled before stitching (seg_summary_kernel, or the host on the slow path)
    int64_t own_lo, own_hi;   // local range of the polished text this segment contributes
    int64_t own_hi0;          // own_hi before this segment's own change of length is added (set when the segment is built)
    int64_t out_off;          // where it goes in the chunk's new text
};
// What the host sets when it cuts a chunk of `len` bases at the positions p_1 < .. < p_m (polish_plan.hpp: fill_chunk), segment
// j = 0 .. m, with W = 4k, M = 3k (CutGeometry), RM = 1 or 8 (the roomy repeat):
//   first = (j == 0), last = (j == m), chain_in = (j > 0 and p_j is a clean-zone boundary), chunk
//   seg_lo = 0 | p_j - W            start_i = 0 | W            stop_orig = p_(j+1) | INT64_MAX
//   len0 = len = min(len, p_(j+1) + M) - seg_lo | len - seg_lo
//   cap = len0 + RM * max(1024, len0 / 8)   (tight: len0 + 2)      gs = 0, glen = cap - len0
//   cls = the chunk's classes (null without a window), cls_n = max(0, len - k + 1)
//   rec_cap = edit_cap = min(2^31 - 1, RM * (2 * len0 / k + 16))    aux_cap = min(2^31 - 1, RM * (2 * len0 + 1024))
//   own_lo = 0 | 2k      own_hi = own_hi0 = (p_(j+1) - 2k) - seg_lo | -1: the owned chunk ranges [p_j - 2k, p_(j+1) - 2k) tile [0, len)
//   buf, recs / edits, aux: consecutive in the three arenas, text and aux in steps of 256 bytes, records by rec_cap
//   arrive = slot 1 + (the segment's index in its table); everything else 0

// what the host needs of a pass's walks, per chunk record (seg_summary_kernel): everything else stays on the device
struct ChunkSummary {
    int64_t newlen;           // length of the chunk's stitched text
    int64_t wrong;            // bad k-mers counted (src/jasper.py:207)
    uint64_t lookups;
    uint32_t nrec, naux;      // fix records / aux bytes of the chunk's segments
    int32_t bad_seg;          // index of the first segment whose status is not PS_OK, or -1
    int32_t spec_fail;        // some segment's speculation failed
};

constexpr long long ARRIVE_PENDING = (long long)0x8080808080808080ull;   // what hipMemset(0x80) leaves
constexpr long long ARRIVE_FAIL = -2, ARRIVE_END = -1;
// what a segment puts into its slot when it STARTS (round 4): CLEAN = chained and nothing can happen in its range, its arrival follows
// from any earlier segment's (successors look past it without waiting for it); WALKING = it walks, its arrival comes at its end
constexpr long long ARRIVE_CLEAN = -3, ARRIVE_WALKING = -4;

struct PolishParams {
    int k;
    int step;       // max(2, round(k/8))            src/jasper.py:20
    uint32_t solid; // solid_thre                    src/jasper.py:23
    int passes;     // P fixing passes; pass P is the QV-only pass (src/jasper.py:25,37-38)
    int fix;
};

// per-chunk arguments of the dense scan / classify / sync-point kernels (one launch covers all chunks of a batch)
struct ScanChunk {
    const uint8_t *text;
    int64_t len;
    uint8_t *cls;
    int64_t *cand;             // sync-point candidates of the WHOLE batch: (chunk << 40) | position, unordered
    unsigned int *cand_count;  // one counter for the batch
    unsigned int cand_cap;
    int32_t want_sync;
    const uint8_t *flags;   // one byte per 64 text positions: the previous pass changed text there (rescan only)
    int64_t *clean_cand;    // per CLEAN_CELL positions: a position whose windows [p-4k, p+k) are all CLEAN, or -1
    uint32_t n_cells;
};
constexpr int64_t CLEAN_CELL = 65536;
// where a pass may cut a chunk (polish_plan.hpp: plan_cuts; jasper_polish_cut_geometry reports the same numbers)
struct CutGeometry {
    int64_t tmin;        // minimum distance between sync points, and from the last one to the chunk end
    int64_t cmin;        // minimum distance between a clean-zone boundary and its neighbours
    int64_t clean_cell;  // one clean-zone boundary candidate per this many positions
    int64_t w;           // clean windows required left of a sync point = text a segment re-reads left of its boundary
    int64_t m;           // text kept right of the next sync point
};
inline CutGeometry cut_geometry(int k) { return CutGeometry{1024, 32768, CLEAN_CELL, 4ll * k, 3ll * k}; }

}  // namespace jk
