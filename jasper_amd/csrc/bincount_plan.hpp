// bincount_plan.hpp -- the host arithmetic of counting chosen reads of a packed batch (bincount.hip): what the host checks of the offsets,
// the bin codes and a sink's mask before a kernel reads them, the list of a sink's reads with where each goes in the sink's stream, how
// that stream is cut into pieces of whole reads, and how large a piece's buffer is.  Plain C++, no HIP: tools/bincount_plan_check.cpp runs
// it under -fsanitize=address,undefined.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace jk {

constexpr int BC_SINKS = 3;                         // sinks of one call at the most
constexpr int BC_BINS = 3;                          // bin codes 0 .. 2, a mask has a bit for each
constexpr uint8_t BC_SEPARATOR = '\n';              // the one non-base byte behind every read of a stream
constexpr uint64_t BC_PIECE = 1ull << 28;           // bytes of a sink's stream gathered and counted at a time (JASPER_BINCOUNT_PIECE overrides it)
constexpr uint64_t BC_PIECE_MOST = 1ull << 36;      // ... and the most the override may ask for
constexpr int64_t BC_MAX_READS = 0x7FFFFFFF;        // reads per call, as the binning takes them (readbins.hpp: RB_MAX_READS)
constexpr int64_t BC_MAX_TEXT = (int64_t)1 << 43;   // text bytes per call (readbins.hpp: RB_MAX_TEXT)
constexpr int BC_THREADS = 256;
constexpr int BC_GROUP = 16;                        // output bytes of a thread: one aligned 16-byte store
constexpr int BC_PAD = 64;                          // separator bytes behind a piece (the counting kernels' 16-byte loads end inside)
enum { BC_OK = 0, BC_BAD_OFFSETS = 1, BC_BAD_CODE = 2, BC_TOO_LARGE = 3, BC_BAD_ARGS = 4 };

inline bool bincount_mask_ok(uint32_t mask) { return mask >= 1 && mask < (1u << BC_BINS); }

// offsets[0] >= 0 and no value below the one before it; every code below BC_BINS; the limits.  The kernel indexes the text by what the
// offsets hold and a mask by a code, so nothing is launched for a batch that fails here.
inline int bincount_check(int64_t n_reads, const int64_t *offsets, const uint8_t *codes) {
    if (n_reads < 0) return BC_BAD_ARGS;
    if (n_reads > BC_MAX_READS) return BC_TOO_LARGE;
    if (n_reads == 0) return BC_OK;
    if (!offsets || !codes) return BC_BAD_ARGS;
    if (offsets[0] < 0) return BC_BAD_OFFSETS;
    for (int64_t i = 0; i < n_reads; ++i) {
        if (offsets[i + 1] < offsets[i]) return BC_BAD_OFFSETS;
        if (codes[i] >= BC_BINS) return BC_BAD_CODE;
    }
    if (offsets[n_reads] - offsets[0] > BC_MAX_TEXT) return BC_TOO_LARGE;
    return BC_OK;
}

// A sink's reads in input order: src[j] = where read j of the sink begins in the text, dst[j] = where it goes in the sink's stream --
// the exclusive scan of (length + 1) over the sink's reads, dst[reads] = the stream's bytes.  A read of any length, 0 included, takes
// its bytes and its separator, so dst increases strictly.
struct SinkList {
    std::vector<int64_t> src;
    std::vector<uint64_t> dst;
    uint64_t reads = 0, bases = 0;
};
inline void sink_list(int64_t n_reads, const int64_t *offsets, const uint8_t *codes, uint32_t mask, SinkList &L) {
    L.src.clear();
    L.dst.clear();
    L.reads = L.bases = 0;
    for (int64_t i = 0; i < n_reads; ++i) L.reads += (mask >> codes[i]) & 1u;
    L.src.reserve((size_t)L.reads);
    L.dst.reserve((size_t)L.reads + 1);
    uint64_t at = 0;
    for (int64_t i = 0; i < n_reads; ++i) {
        if (!((mask >> codes[i]) & 1u)) continue;
        L.src.push_back(offsets[i]);
        L.dst.push_back(at);
        at += (uint64_t)(offsets[i + 1] - offsets[i]) + 1;
    }
    L.dst.push_back(at);
    L.bases = at - L.reads;
}

// The piece that begins with read j0 of the list (j0 < reads) ends before read j1: the most whole reads whose bytes and separators fit
// `piece` bytes, and one read when the first alone does not fit.  No k-mer is lost at a seam, since no read is cut.
inline uint64_t piece_end(const std::vector<uint64_t> &dst, uint64_t j0, uint64_t piece) {
    const uint64_t reads = dst.size() - 1;
    const uint64_t limit = dst[j0] + piece;
    const uint64_t j1 = (uint64_t)(std::upper_bound(dst.begin() + (ptrdiff_t)j0, dst.end(), limit) - dst.begin()) - 1;      // the last j with dst[j] <= limit
    return std::min(std::max(j1, j0 + 1), reads);
}
// bytes of the largest piece of a list: what the piece buffer has to hold of the stream
inline uint64_t largest_piece(const std::vector<uint64_t> &dst, uint64_t piece) {
    uint64_t most = 0;
    for (uint64_t j0 = 0, reads = dst.size() - 1; j0 < reads;) {
        const uint64_t j1 = piece_end(dst, j0, piece);
        most = std::max(most, dst[j1] - dst[j0]);
        j0 = j1;
    }
    return most;
}
// 16-byte groups the kernel writes for a piece of `bytes` bytes (the piece, filled up to a whole group, and BC_PAD separator bytes),
// the buffer's bytes and the workgroups of the launch
inline uint64_t piece_groups(uint64_t bytes) { return (bytes + BC_GROUP - 1) / BC_GROUP + BC_PAD / BC_GROUP; }
inline size_t piece_room(uint64_t bytes) { return (size_t)(piece_groups(bytes) * BC_GROUP); }
inline uint64_t piece_blocks(uint64_t bytes) { return (piece_groups(bytes) + BC_THREADS - 1) / BC_THREADS; }

// JASPER_BINCOUNT_PIECE=<bytes>: 1 .. BC_PIECE_MOST in decimal digits; false for anything else
inline bool piece_from_text(const char *v, uint64_t &piece) {
    if (!v || !*v) return false;
    uint64_t n = 0;
    for (const char *p = v; *p; ++p) {
        if (*p < '0' || *p > '9' || n > BC_PIECE_MOST) return false;
        n = n * 10 + (uint64_t)(*p - '0');
    }
    if (n < 1 || n > BC_PIECE_MOST) return false;
    piece = n;
    return true;
}

}  // namespace jk
