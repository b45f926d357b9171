// polish.hpp -- what the polishing kernels (polish.hip) offer the host (polish_host.hip); the plain structs are in polish_types.hpp.
#pragma once
#include "polish_types.hpp"
#include "table.hpp"

namespace jk {

// scratch of the path-extension search (src/jasper.py:527-583), pooled: a wave takes a slot only while it searches
struct ScratchPool {
    unsigned int *locks;   // 0 free, 1 taken
    uint8_t *base;
    size_t stride;         // bytes per slot
    uint32_t nslots;
    uint32_t node_cap;     // trie arena entries (uint32)
    uint32_t front_cap;    // frontier entries (80 B)
    uint32_t patch_cap;    // bytes
    size_t off_front, off_patch;
};

// pass 0: dense scan (counts stay in LDS) + classes + sync-point candidates of every chunk
void launch_scan_batch(const TableDev &T, const ScanChunk *d_chunks, int n_chunks, int k, uint32_t solid, hipStream_t stream);
// later passes: classes were carried over by the stitch; recompute the 64-window tiles next to changed text, then candidates
void launch_rescan_batch(const TableDev &T, const ScanChunk *d_chunks, int n_chunks, int k, uint32_t solid, hipStream_t stream);

void launch_copy_chunks(uint8_t *const *d_chunk_ptr, uint8_t *d_pack, const int64_t *d_offs, int n, bool to_chunks, hipStream_t stream);
// The kernels around the walk take a flat list of (segment, 4 KiB piece) -- make_pieces() -- one block each.  A segment's pieces
// are cut from the lengths the host knows when it builds the table; whatever lies beyond them (the text a walk added, the margins of
// the segment's private copy) falls to the piece marked as its last.
constexpr int64_t SEG_PIECE = 4096;
constexpr uint32_t SEG_PIECE_LAST = 0x80000000u;
struct SegPiece {
    uint32_t seg;
    uint32_t piece;        // | SEG_PIECE_LAST
};
// pieces of n_segs segments appended to out; returns how many
inline size_t make_pieces(const SegDev *segs, size_t n_segs, SegPiece *out) {
    size_t n = 0;
    for (size_t s = 0; s < n_segs; ++s) {
        const int64_t own = (segs[s].last ? segs[s].len0 : segs[s].own_hi0) - segs[s].own_lo;
        const uint32_t np = own > SEG_PIECE ? (uint32_t)((own + SEG_PIECE - 1) / SEG_PIECE) : 1u;
        for (uint32_t p = 0; p < np; ++p) out[n++] = SegPiece{(uint32_t)s, p + 1 == np ? (p | SEG_PIECE_LAST) : p};
    }
    return n;
}
inline size_t max_pieces(size_t max_segs, size_t text_bytes) { return max_segs + text_bytes / (size_t)SEG_PIECE + 1; }

// what seg_init_kernel presets besides the segments' texts, so that a pass puts no fills on its stream
struct PassPreset {
    long long *arrive;         // n_arrive slots (the segments' and the two guard slots) become ARRIVE_PENDING
    int64_t n_arrive;
    unsigned int *ticket;      // the walk's ticket: 0
    unsigned int *cand_count;  // the scan's candidate count for the NEXT pass: 0 (this pass's has been fetched); may be null
    uint8_t *flags;            // changed-text flags, n_flag16 * 16 bytes: 0 (this pass's rescan has read them; the stitch sets them)
    int64_t n_flag16;
};
void launch_seg_init(const SegDev *d_segs, const SegPiece *d_work, int n_work, const uint8_t *const *d_chunk_text, const PassPreset &preset,
                     hipStream_t stream);
// d_ticket: one device word, zero (seg_init_kernel); d_segs[i].arrive must point into an array preset to ARRIVE_PENDING (the same)
void launch_seg_walk(const TableDev &T, SegDev *d_segs, int n_segs, PolishParams pp, int pass, ScratchPool pool, unsigned int *d_ticket,
                     hipStream_t stream);
// After the walks: per chunk (its segments are consecutive, in text order) the stitched coordinates -- own_hi / out_off of every
// segment written back into d_segs -- the coordinate bases the gather needs (idx_base, seq_base, rec_off, aux_off: n_segs each;
// rec_off / aux_off count from the CHUNK's first record / aux byte) and one ChunkSummary per chunk.
// first_seg[c] .. first_seg[c+1] = the chunk's segments.
void launch_seg_summary(SegDev *d_segs, int n_segs, const int32_t *d_first_seg, int n_chunks, int64_t *idx_base, uint32_t *seq_base, uint32_t *rec_off,
                        uint32_t *aux_off, ChunkSummary *d_out, hipStream_t stream);
// Gather of the fix records / aux bytes and stitch of the new text in one launch.  d_cls_out / d_flags may be null (last pass): then
// only the text is stitched.  out_recs null: nothing to gather.  d_sum: the summaries launch_seg_summary left (rec_off / aux_off
// relative to the chunk), or null when rec_off / aux_off are offsets into out_recs / out_aux (the host's bookkeeping).
void launch_seg_finish(const SegDev *d_segs, int n_segs, const SegPiece *d_work, int n_work, uint8_t *const *d_chunk_out, uint8_t *const *d_cls_out,
                       uint8_t *const *d_flags, const int64_t *idx_base, const uint32_t *seq_base, const uint32_t *rec_off, const uint32_t *aux_off,
                       const ChunkSummary *d_sum, FixRec *out_recs, uint8_t *out_aux, hipStream_t stream);

}  // namespace jk
