// deflate_gpu.hpp -- text in HBM -> BGZF members (deflate_gpu.hip): what `triobin --write-gz --deflate device` writes its bin files with.
//
// An extension: the reference has no counterpart.  The n text bytes are cut into blocks of DF_BLOCK bytes (the last may be short), every
// block becomes one complete gzip member with the BGZF extra field, and the members lie back to back in the output.  n = 0 gives no
// member; the empty member that ends a BGZF file is the file writer's.  Semantics: include/jasper_hip.h (jasper_deflate_bgzf).
#pragma once
#include "deflate_plan.hpp"
#include "table.hpp"
#include <string>

namespace jk {

// Compress the n bytes at d_text (any alignment; T's device) on T's stream.  out (host, room for out_cap bytes) gets the members, *out_bytes
// how many bytes; a call whose members do not fit out_cap fails and writes nothing.  counters[DF_COUNTERS] and *seconds (device time of the
// kernels by HIP events; may be null) are ADDED to.  Buffers: T's workspace slots WS_DEFLATE + 1 ..; d_text may lie in WS_DEFLATE + 0.
int deflate_device(Table &T, const uint8_t *d_text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_bytes, uint64_t *counters, double *seconds, std::string &err);
// the same with the text in host memory: it is uploaded to WS_DEFLATE + 0, at its host pointer's place within 16 bytes; counters and seconds are SET
int deflate_host(Table &T, const uint8_t *text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_bytes, uint64_t *counters, double *seconds, std::string &err);

}  // namespace jk
