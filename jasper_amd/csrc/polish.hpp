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
void launch_seg_init(SegDev *d_segs, int n_segs, const uint8_t *const *d_chunk_text, hipStream_t stream);
// d_ticket: one device word (zeroed by the call); d_segs[i].arrive must point into an array preset to ARRIVE_PENDING
void launch_seg_walk(const TableDev &T, SegDev *d_segs, int n_segs, PolishParams pp, int pass, ScratchPool pool, unsigned int *d_ticket,
                     hipStream_t stream);
// d_cls_out / d_flags may be null (last pass): then only the text is stitched
void launch_seg_stitch(const SegDev *d_segs, int n_segs, uint8_t *const *d_chunk_out, uint8_t *const *d_cls_out, uint8_t *const *d_flags,
                       hipStream_t stream);
// After the walks: per chunk (its segments are consecutive, in text order) the stitched coordinates -- own_hi / out_off of every
// segment written back into d_segs -- the coordinate bases the gather needs (idx_base, seq_base, rec_off, aux_off: n_segs each)
// and one ChunkSummary per chunk.  first_seg[c] .. first_seg[c+1] = the chunk's segments.
void launch_seg_summary(SegDev *d_segs, int n_segs, const int32_t *d_first_seg, int n_chunks, int64_t *idx_base, uint32_t *seq_base, uint32_t *rec_off,
                        uint32_t *aux_off, ChunkSummary *d_out, hipStream_t stream);
void launch_seg_gather(const SegDev *d_segs, int n_segs, const int64_t *idx_base, const uint32_t *seq_base, const uint32_t *rec_off,
                       const uint32_t *aux_off, FixRec *out_recs, uint8_t *out_aux, hipStream_t stream);

}  // namespace jk
