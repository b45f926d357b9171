// readroute.hpp -- the second pass of `triobin --write-reads` on the GPU (readroute.hip): a block of file text in HBM cut into segments,
// every segment's bytes moved to the output of its bin.
//
// An extension: the reference has no counterpart.  The text's n bytes are cut by bounds[n_seg + 1] (bounds[0] = 0, bounds[n_seg] = n,
// never decreasing; a segment may be empty), segment i has bin code bins[i] in 0..2.  The kernels write the segments of each bin back to
// back in input order and the three byte totals; every text byte leaves exactly once.  Semantics: include/jasper_hip.h (jasper_route_text).
#pragma once
#include "readroute_plan.hpp"
#include "table.hpp"
#include <string>

namespace jk {

// how a text is cut and what is checked: mismatches = the segments i >= check_from that hold a byte and whose first byte is not `first`
struct RouteJob {
    int64_t n_seg;
    const int64_t *bounds;
    const uint8_t *bins;
    int first;
    int check_from;
};
// Where the three bins go (all host memory).  out_cap == nullptr: plain bytes -- out[b] (room for n bytes each) gets bin b's bytes,
// out_bytes[b] how many; raw_bytes and counters are not looked at.  Otherwise BGZF members (deflate_gpu.hpp): the routed bytes stay in
// HBM, the compressor runs on each bin's range and only the members are copied down to out[b] (room for out_cap[b] bytes); out_bytes[b] =
// the members' bytes, raw_bytes[b] = the routed bytes, counters[DF_COUNTERS] (may be null) = the three compressor calls' sums.  A bin
// without a byte gets no member.
struct RouteOut {
    uint8_t *const *out;
    const int64_t *out_cap;
    int64_t *out_bytes;
    int64_t *raw_bytes;
    int64_t *mismatches;
    uint64_t *counters;
};
// device time by HIP events: the route kernels, a session's pull of inflated text (readgz.hpp), the compressor's kernels.  A call zeroes
// the ones it can fill once it has accepted the arguments they belong to
struct RouteSeconds {
    double route, pull, deflate;
};

// Route the n bytes at `text` (any alignment) on T's stream.  on_device: the text lies on T's device (it may lie in WS_ROUTE + 0);
// otherwise it is host memory and is uploaded to WS_ROUTE + 0, at its host pointer's place within 16 bytes.  Buffers: T's workspace slots
// WS_ROUTE + 1 ..
int route_text(Table &T, const uint8_t *text, bool on_device, int64_t n, const RouteJob &J, const RouteOut &O, RouteSeconds &S, std::string &err);
// room for n text bytes in WS_ROUTE + 0 (what a caller that fills the text itself asks for first)
uint8_t *route_text_room(Table &T, int64_t n, std::string &err);

}  // namespace jk
