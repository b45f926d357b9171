// readroute.hip -- a block of file text in HBM, cut into segments that each carry a bin code -> the segments of each bin back to back
// (semantics: include/jasper_hip.h, jasper_route_text; the host code it replaces: jasper_amd/triobin.py, _write_reads_by_starts, whose
// three boolean-mask gathers touch every text byte three times on one core).
//
//   rr_sizes_kernel   one thread per segment: its size into its bin's column, 0 into the two others; and the check -- a segment
//                     i >= check_from that holds a byte and does not begin with `first` is counted (the second pass's "a remembered start
//                     no longer holds @ / >")
//   rt_scan_words     (readtext.hip) three exclusive scans: pre[b][i] = bytes of bin b before segment i, pre[b][n_seg] = bin b's total
//   rr_copy_kernel    by TEXT bytes, 16 per thread, as rt_pack_kernel moves sequence lines: one binary search in bounds for the segment
//                     the thread's first byte lies in, then a walk over the segments its 16 bytes touch.  16 bytes inside one segment
//                     leave in one 16-byte store (global stores need no alignment on gfx950), the others byte by byte.  A 100 kb record
//                     is spread over many workgroups this way.  The three outputs lie back to back in one buffer of n bytes -- bin 1
//                     begins where bin 0's total ends -- so the kernel reads the text once and writes n bytes once
// The host stage is route_text: what is refused (route_refuse), the upload of a host text, the kernels (route_core) and what leaves the GPU
// (route_finish: the three ranges, or their BGZF members).  It waits once, for the three totals and the check's count; they say how much
// of the output buffer goes where.
#include "readroute.hpp"
#include "deflate_gpu.hpp"
#include "readtext.hpp"
#include "scan_tile.hpp"

namespace jk {

namespace {

enum { RRC_MISMATCH = 0, RRC_WORDS = 2 };

__global__ __launch_bounds__(RT_THREADS) void rr_sizes_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ bounds, const uint8_t *__restrict__ bins,
                                                              uint64_t n_seg, uint64_t col_words, uint32_t first, uint64_t check_from, uint64_t *__restrict__ cols,
                                                              unsigned long long *__restrict__ ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (i >= n_seg) return;
    const uint64_t s = (uint64_t)bounds[i], size = (uint64_t)bounds[i + 1] - s;
    const uint32_t b = bins[i];
    cols[i] = b == 0 ? size : 0;
    cols[col_words + i] = b == 1 ? size : 0;
    cols[2 * col_words + i] = b == 2 ? size : 0;
    if (i >= check_from && size && text[s] != first) atomicAdd(&ctl[RRC_MISMATCH], 1ull);      // (s < n: the segment holds a byte)
}

__global__ __launch_bounds__(RT_THREADS) void rr_copy_kernel(const uint8_t *__restrict__ text, uint64_t n, const int64_t *__restrict__ bounds, const uint8_t *__restrict__ bins,
                                                             uint64_t n_seg, const uint64_t *__restrict__ pre, uint64_t pre_words, uint8_t *__restrict__ out) {
    const uint64_t pos = (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16;
    if (pos >= n) return;
    const Raw16 r = load16(text, (int64_t)pos, (int64_t)n);
    // the segment my first byte lies in: the last one that begins at or before it and does not end there.  bounds[n_seg] = n > pos
    uint64_t lo = 1, hi = n_seg;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)bounds[mid] > pos) hi = mid;
        else lo = mid + 1;
    }
    uint64_t seg = lo - 1;
    const uint64_t base1 = pre[n_seg], base2 = base1 + pre[pre_words + n_seg];      // where bins 1 and 2 begin in out
    uint64_t s = 0, e = 0, dst = 0;
    auto open_seg = [&]() {
        const uint32_t b = bins[seg];
        s = (uint64_t)bounds[seg];
        e = (uint64_t)bounds[seg + 1];
        dst = (b == 0 ? 0 : b == 1 ? base1 : base2) + pre[b * pre_words + seg];
    };
    open_seg();
    if (pos + 16 <= e) {
        struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
        V16 v;
        v.w[0] = r.w[0]; v.w[1] = r.w[1]; v.w[2] = r.w[2]; v.w[3] = r.w[3];
        *reinterpret_cast<V16 *>(out + dst + (pos - s)) = v;
        return;
    }
    for (int j = 0; j < 16; ++j) {
        const uint64_t p = pos + j;
        if (p >= n) break;
        while (p >= e) {                                // (empty segments are stepped over; p < n = bounds[n_seg] ends it)
            ++seg;
            open_seg();
        }
        out[dst + (p - s)] = (uint8_t)((r.w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    }
}

const char *const RR_WHAT = "route text";

}  // namespace

uint8_t *route_text_room(Table &T, int64_t n, std::string &err) {
    if (n < 0 || n > RT_MAX_TEXT) { err = std::string(RR_WHAT) + ": more than 2^31-1 text bytes in one call"; return nullptr; }
    return (uint8_t *)T.workspace(Table::WS_ROUTE, route_buffers((uint64_t)n, 0).text, err);
}

namespace {
// what is refused before anything is queued, and the outputs' initial state: the compressed outputs' arguments, the others, then
// route_check's verdict in words
int route_refuse(int64_t n, const RouteJob &J, const RouteOut &O, RouteSeconds &S, std::string &err) {
    const std::string w(RR_WHAT);
    if (O.out_cap) {
        if (!O.raw_bytes) { err = w + ": bad arguments"; return -1; }
        O.raw_bytes[0] = O.raw_bytes[1] = O.raw_bytes[2] = 0;
        if (O.counters)
            for (int i = 0; i < DF_COUNTERS; ++i) O.counters[i] = 0;
        S.deflate = 0;
    }
    if (!O.out_bytes || !O.mismatches || !O.out || (J.check_from != 0 && J.check_from != 1) || J.first < 0 || J.first > 255) { err = w + ": bad arguments"; return -1; }
    O.out_bytes[0] = O.out_bytes[1] = O.out_bytes[2] = 0;
    *O.mismatches = 0;
    S.route = 0;
    switch (route_check(n, J.n_seg, J.bounds, J.bins)) {
    case RR_TOO_LARGE: err = w + ": more than 2^31-1 text bytes or segments in one call"; return -1;
    case RR_BAD_BOUNDS: err = w + ": bounds must begin with 0, end with n and never decrease"; return -1;
    case RR_BAD_BIN: err = w + ": a bin code is not 0, 1 or 2"; return -1;
    default: return 0;
    }
}

// the kernels, for segments route_refuse has let pass (n > 0): the routed bytes stay in HBM, bin b's tot[b] bytes behind those of the bins
// before it from *d_routed on; the one wait of the path is here
int route_core(Table &T, const uint8_t *d_text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t **d_routed,
               uint64_t tot[RR_BINS], int64_t *mismatches, double *seconds, std::string &err) {
    const std::string w(RR_WHAT);
    HIPCHK(hipSetDevice(T.device));
    hipStream_t st = T.stream;
    const uint64_t un = (uint64_t)n, ns = (uint64_t)n_seg;
    const RouteBuffers B = route_buffers(un, ns);
    const uint64_t cw = route_col_words(ns), pw = route_pre_words(ns), bw = route_block_words(ns);
    const int W = Table::WS_ROUTE;
    int64_t *d_bounds = (int64_t *)T.workspace(W + 1, B.bounds, err);
    uint8_t *d_bins = (uint8_t *)T.workspace(W + 2, B.bins, err);
    uint64_t *d_cols = (uint64_t *)T.workspace(W + 3, B.cols, err);
    uint64_t *d_pre = (uint64_t *)T.workspace(W + 4, B.pre, err);
    uint64_t *d_blk = (uint64_t *)T.workspace(W + 5, B.blocks, err);
    uint8_t *d_out = (uint8_t *)T.workspace(W + 6, B.out, err);
    unsigned long long *d_ctl = (unsigned long long *)T.workspace(W + 7, RRC_WORDS * sizeof(unsigned long long), err);
    if (!d_bounds || !d_bins || !d_cols || !d_pre || !d_blk || !d_out || !d_ctl) return -1;
    HIPCHK(hipMemcpyAsync(d_bounds, bounds, (size_t)(ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_bins, bins, (size_t)ns, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_ctl, 0, RRC_WORDS * sizeof(unsigned long long), st));
    Events ev;
    if (ev.create(err)) return -1;
    HIPCHK(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(rr_sizes_kernel, dim3((unsigned)((ns + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, st, d_text, d_bounds, d_bins, ns, cw, (uint32_t)first,
                       (uint64_t)check_from, d_cols, d_ctl);
    HIPCHK(hipGetLastError());
    for (int b = 0; b < RR_BINS; ++b)
        if (rt_scan_words(st, d_cols + b * cw, ns, d_blk + b * bw, d_pre + b * pw, err)) return -1;
    hipLaunchKernelGGL(rr_copy_kernel, dim3((unsigned)rt_blocks(un)), dim3(RT_THREADS), 0, st, d_text, un, d_bounds, d_bins, ns, d_pre, pw, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    tot[0] = tot[1] = tot[2] = 0;
    unsigned long long bad = 0;
    for (int b = 0; b < RR_BINS; ++b) HIPCHK(hipMemcpyAsync(&tot[b], d_pre + b * pw + ns, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bad, d_ctl + RRC_MISMATCH, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) *seconds = s;
    if (tot[0] + tot[1] + tot[2] != un) { err = w + ": the scans left totals that are not the text's length"; return -1; }
    *mismatches = (int64_t)bad;
    *d_routed = d_out;
    return 0;
}

// what leaves the GPU: the three ranges as they are, or the compressor on each of them and its members
int route_finish(Table &T, const uint8_t *d_routed, const uint64_t tot[RR_BINS], const RouteOut &O, RouteSeconds &S, std::string &err) {
    hipStream_t st = T.stream;
    uint64_t at = 0;
    for (int b = 0; b < RR_BINS; ++b) {
        if (O.out_cap) {
            if (deflate_device(T, d_routed + at, (int64_t)tot[b], O.out[b], O.out_cap[b], &O.out_bytes[b], O.counters, &S.deflate, err)) return -1;
            O.raw_bytes[b] = (int64_t)tot[b];
        } else {
            if (tot[b]) HIPCHK(hipMemcpyAsync(O.out[b], d_routed + at, (size_t)tot[b], hipMemcpyDeviceToHost, st));
            O.out_bytes[b] = (int64_t)tot[b];
        }
        at += tot[b];
    }
    if (!O.out_cap) HIPCHK(jk_stream_wait(st));         // (the compressor has waited for its members)
    return 0;
}
}  // namespace

int route_text(Table &T, const uint8_t *text, bool on_device, int64_t n, const RouteJob &J, const RouteOut &O, RouteSeconds &S, std::string &err) {
    if (route_refuse(n, J, O, S, err)) return -1;
    const uint8_t *d_text = on_device ? text : nullptr;
    if (!on_device && n > 0) {
        if (!text) { err = std::string(RR_WHAT) + ": null text"; return -1; }
        HIPCHK(hipSetDevice(T.device));
        uint8_t *room = route_text_room(T, n, err);
        if (!room) return -1;
        uint8_t *up = room + ((uintptr_t)text & 15u);   // (the kernels take any alignment; the tests reach every one through the host pointer)
        HIPCHK(hipMemcpyAsync(up, text, (size_t)n, hipMemcpyHostToDevice, T.stream));
        d_text = up;
    }
    if (n == 0) return 0;
    if (!d_text || !O.out[0] || !O.out[1] || !O.out[2]) { err = std::string(RR_WHAT) + ": bad arguments"; return -1; }
    uint8_t *d_out = nullptr;
    uint64_t tot[RR_BINS];
    int64_t bad = 0;
    if (route_core(T, d_text, n, J.n_seg, J.bounds, J.bins, J.first, J.check_from, &d_out, tot, &bad, &S.route, err)) return -1;
    if (route_finish(T, d_out, tot, O, S, err)) return -1;
    *O.mismatches = bad;
    return 0;
}

}  // namespace jk
