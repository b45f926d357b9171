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

// Route the n bytes at d_text (any alignment; T's device) on T's stream.  out[b] (host, room for n bytes each) gets bin b's bytes,
// out_bytes[b] how many.  mismatches = the segments i >= check_from that hold a byte and whose first byte is not `first`.  seconds
// (may be null) = device time of the kernels (HIP events).  Buffers: T's workspace slots WS_ROUTE + 1 ..; d_text may lie in WS_ROUTE + 0.
int route_text_device(Table &T, const uint8_t *d_text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *const out[3],
                      int64_t out_bytes[3], int64_t *mismatches, double *seconds, std::string &err);
// the same with the text in host memory: it is uploaded to WS_ROUTE + 0, at its host pointer's place within 16 bytes
int route_text_host(Table &T, const uint8_t *text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *const out[3],
                    int64_t out_bytes[3], int64_t *mismatches, double *seconds, std::string &err);
// The same two, but out[b] (host, room for out_cap[b] bytes) gets bin b's bytes as BGZF members (deflate_gpu.hpp): the routed bytes stay in
// HBM, the compressor runs on each bin's range and only the members are copied down.  out_bytes[b] = the members' bytes, raw_bytes[b] =
// the routed bytes; counters[DF_COUNTERS] (may be null) = the three compressor calls' sums; seconds[2] (may be null) = the route kernels,
// the compressor's kernels.  A bin without a byte gets no member.
int route_text_device_gz(Table &T, const uint8_t *d_text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *const out[3],
                         const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *mismatches, uint64_t *counters, double *seconds, std::string &err);
int route_text_host_gz(Table &T, const uint8_t *text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *const out[3],
                       const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *mismatches, uint64_t *counters, double *seconds, std::string &err);
// room for n text bytes in WS_ROUTE + 0 (what a caller that fills the text itself asks for first)
uint8_t *route_text_room(Table &T, int64_t n, std::string &err);

}  // namespace jk
