// readgz.hpp -- a gzip text session for the trio read binning (readgz.hip): ONE .gz read file inflated on the GPU (inflate_gpu.hpp) whose
// text goes from the inflater to the read-text path (readtext.hpp) or to the routing path (readroute.hpp) inside HBM.
//
// An extension: the reference has no counterpart.  The session belongs to one table: the inflater runs on that table's device and
// stream, its five buffers are the table's WS_GZ slots, the text of a call lies in the table's WS_READTEXT slot (bins) or WS_ROUTE slot
// (route).  No counting call may run on that table while a session is open.  Semantics: include/jasper_hip.h (jasper_gz_text_open).
#pragma once
#include "inflate_gpu.hpp"
#include "readroute.hpp"
#include "readtext.hpp"
#include <memory>
#include <string>

namespace jk {

constexpr int RT_NO_FORMAT = 2;     // status of gz_text_bins: the text's first byte is neither '@' nor '>'; nothing was parsed

struct GzText {
    Table *M = nullptr;
    uint64_t stats[GZS_N] = {0, 0, 0, 0, 0, 0};
    std::unique_ptr<DeviceGunzip> dg;
    uint8_t *d_tail = nullptr;      // the unused end of the last bins call's text (a buffer of the session's own: the text slot is written from its front)
    size_t tail_cap = 0;
    int64_t tail = 0;
    int64_t n = -1;                 // bytes of the current bins call's text, -1: there is none
    int mode = 0;                   // 0 fresh, 1 a bins session, 2 a route session: one pass over the file is one or the other (route has no tail)
    ~GzText();
};

// null with err set when DeviceGunzip::open refuses the file (not a regular file, no valid gzip header, no memory)
GzText *gz_text_open(Table &M, const char *path, std::string &err);
// format: 0 = decide from the text's first byte, 1 = FASTQ, 2 = FASTA (in / out).  seconds[3]: read_text_core's two, then the pull's:
// HIP events around read_device, so the inflater's kernels and copies AND the host's stitching and waits between them -- the stream's
// time from the pull's first command to its last, which is what the call spends on inflating, not kernel time alone.
// The text of a bins call lies in the table's WS_READTEXT slot: gz_text_copy reads it from there, so it is to be called before any other
// read-text call on that table (which overwrites the slot; the carried tail is safe in the session's own buffer).
int gz_text_bins(GzText &G, Table &M, Table &P, int64_t want, int *format, uint32_t thre_mat, uint32_t thre_pat, int64_t *n, int *eof, int64_t *used, int64_t *n_records,
                 int *status, int64_t *bad_record, double *seconds, std::string &err);
int gz_text_copy(GzText &G, int64_t from, int64_t len, uint8_t *dst, std::string &err);
// The next `want` inflated bytes pulled into the routing path's text slot, *got of them, and routed there by route_text (readroute.hpp: the
// outputs plain or as BGZF members) when *got is what the bounds end with; otherwise nothing is routed.  S is zeroed first; S.pull is timed
// as above.  Refused on a session that has served a bins call, and bins on one that has routed
int gz_text_route(GzText &G, Table &T, int64_t want, const RouteJob &J, const RouteOut &O, int64_t *got, RouteSeconds &S, std::string &err);

}  // namespace jk
