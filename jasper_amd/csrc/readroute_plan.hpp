// readroute_plan.hpp -- the host arithmetic of the routing path (readroute.hip): what the host checks of a block's segments before a
// kernel reads them, and how large every buffer of the path is.  Plain C++, no HIP: tools/readroute_plan_check.cpp runs it under
// -fsanitize=address,undefined.
#pragma once
#include "readtext_plan.hpp"

namespace jk {

constexpr int RR_BINS = 3;
constexpr int64_t RR_MAX_SEGMENTS = 0x7FFFFFFF;
enum { RR_OK = 0, RR_BAD_BOUNDS = 1, RR_BAD_BIN = 2, RR_TOO_LARGE = 3 };

// bounds[0] = 0, bounds[n_seg] = n, no value below the one before it; every bin code below RR_BINS.  The kernels index the text and the
// three columns by what these arrays hold, so nothing is launched for a block that fails here.
inline int route_check(int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins) {
    if (n < 0 || n > RT_MAX_TEXT || n_seg < 0 || n_seg > RR_MAX_SEGMENTS) return RR_TOO_LARGE;
    if (!bounds || bounds[0] != 0 || bounds[n_seg] != n) return RR_BAD_BOUNDS;
    for (int64_t i = 0; i < n_seg; ++i) {
        if (bounds[i + 1] < bounds[i]) return RR_BAD_BOUNDS;
        if (!bins || bins[i] >= RR_BINS) return RR_BAD_BIN;
    }
    return RR_OK;
}

// bytes of the path's buffers
struct RouteBuffers {
    size_t text = 0;        // the text, up to 15 bytes before it (it keeps its host pointer's place within 16 bytes) and its padding
    size_t bounds = 0;      // int64 per segment and one more
    size_t bins = 0;        // a byte per segment
    size_t cols = 0;        // three columns of uint64 per segment: a segment's size in its bin's column, 0 in the others
    size_t pre = 0;         // their exclusive scans, each with the bin's total behind it
    size_t blocks = 0;      // per column: uint64 per block of the scan and one for the total
    size_t out = 0;         // the three outputs back to back: the text's bytes, each once
};
inline size_t route_col_words(uint64_t n_seg) { return (size_t)(n_seg ? n_seg : 1); }      // (a column is never empty: the scan is handed a pointer)
inline size_t route_pre_words(uint64_t n_seg) { return (size_t)(n_seg + 1); }
inline size_t route_block_words(uint64_t n_seg) { return (size_t)(rt_blocks(n_seg) + 1); }
inline RouteBuffers route_buffers(uint64_t n, uint64_t n_seg) {
    RouteBuffers b;
    b.text = (size_t)n + 15 + RT_PAD;
    b.bounds = (size_t)(n_seg + 1) * sizeof(int64_t);
    b.bins = (size_t)(n_seg ? n_seg : 1);
    b.cols = RR_BINS * route_col_words(n_seg) * sizeof(uint64_t);
    b.pre = RR_BINS * route_pre_words(n_seg) * sizeof(uint64_t);
    b.blocks = RR_BINS * route_block_words(n_seg) * sizeof(uint64_t);
    b.out = (size_t)n + RT_PAD;
    return b;
}

}  // namespace jk
