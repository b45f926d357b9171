// bincount.hip -- chosen reads of a packed batch -> the base stream Table::count_device takes -> a table per sink (semantics:
// include/jasper_hip.h, jasper_count_binned; the host arithmetic: bincount_plan.hpp).
//
// An extension the reference has no counterpart for.  count(own bin + unknown) = count(all reads) - count(other bin), key by key, so
// the k-mer database a haplotype is polished with needs only the two small bins counted while the batch is in HBM (triobin --write-jf;
// the subtraction: select.hip, table_subtract).
//
//   reads_gather_kernel   by OUTPUT bytes, 16 per thread, the mirror of rt_pack_kernel and rr_copy_kernel (which cut the input): a
//                         thread owns one aligned 16-byte group of the piece, finds the read its first byte lies in by one binary
//                         search in the sink's destination offsets -- within the piece's reads -- and, where all 16 bytes are bases
//                         of that read, loads them from the unaligned source in one 16-byte load.  A group that holds a separator
//                         or a seam between reads is put together byte by byte, over as many reads as it touches (empty reads are
//                         a separator each).  Either way the group leaves in ONE 16-byte store: plain vector stores, no lane waits
//                         for another, no atomics.  Behind the piece the kernel writes separators up to the buffer's end, so
//                         whatever the counting kernels load behind their last base is a non-base byte this call has written.
// The host stage: the batch is checked once (bincount_check), then sink by sink the list of its reads (sink_list), the two lists
// uploaded, and per piece the gather and Table::count_device on the sink's own stream and in the sink's own workspace.  count_device
// returns when the piece is in the table, so the one piece buffer is free for the next gather; the gather's events are read then.
#include "bincount.hpp"
#include "readtext.hpp"
#include "scan_tile.hpp"
#include <chrono>
#include <cstdlib>

namespace jk {

namespace {

struct __attribute__((packed, aligned(1))) U16 { uint32_t w[4]; };      // 16 bytes at any address

// src[j], dst[j] for the sink's reads j0 .. j1 (dst[j1] = the piece's end); out: piece_room(dst[j1] - dst[j0]) bytes, 16-byte aligned
__global__ __launch_bounds__(BC_THREADS) void reads_gather_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ src, const uint64_t *__restrict__ dst,
                                                                  uint64_t j0, uint64_t j1, uint64_t groups, uint8_t *__restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x;
    if (g >= groups) return;
    const uint64_t pos = g * BC_GROUP;
    const uint64_t base = dst[j0], bytes = dst[j1] - base;
    const uint32_t sep4 = BC_SEPARATOR * 0x01010101u;
    uint4 v = make_uint4(sep4, sep4, sep4, sep4);
    if (pos < bytes) {
        // the read my first byte lies in: the last j of j0 .. j1 - 1 with dst[j] <= base + pos (dst increases strictly)
        uint64_t lo = j0, hi = j1 - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (dst[mid] - base <= pos) lo = mid;
            else hi = mid - 1;
        }
        uint64_t j = lo;
        uint64_t s = dst[j] - base, e = dst[j + 1] - base - 1;      // the read's bases are [s, e) of the piece, its separator is at e
        if (pos + BC_GROUP <= e) {
            const U16 r = *reinterpret_cast<const U16 *>(text + src[j] + (int64_t)(pos - s));
            v = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
        } else {
            uint32_t w[4] = {sep4, sep4, sep4, sep4};
            const uint8_t *from = text + src[j];
            for (int b = 0; b < BC_GROUP; ++b) {
                const uint64_t p = pos + b;
                if (p >= bytes) break;
                if (p > e) {                            // (one step: a read ends with its separator, the next begins right behind it)
                    ++j;
                    s = e + 1;
                    e = dst[j + 1] - base - 1;
                    from = text + src[j];
                }
                if (p < e) w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)from[p - s] << (8 * (b & 3)));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    *reinterpret_cast<uint4 *>(out + pos) = v;
}

const char *const BC_WHAT = "count binned";

int piece_bytes(uint64_t &piece, std::string &err) {
    piece = BC_PIECE;
    const char *v = getenv("JASPER_BINCOUNT_PIECE");
    if (!v) return 0;
    if (!piece_from_text(v, piece)) { err = std::string(BC_WHAT) + ": JASPER_BINCOUNT_PIECE must be a number of bytes from 1 to " + std::to_string(BC_PIECE_MOST); return -1; }
    return 0;
}

// what every entry refuses of the sinks before anything is uploaded, and the outputs' initial state; `like` (may be null) is a table
// the sinks must share k and device with
int check_sinks(const BinSinks &S, Table *like, Table *const *keep, int n_keep, std::string &err) {
    const std::string w(BC_WHAT);
    if (S.n < 1 || S.n > BC_SINKS || !S.tables || !S.masks || !S.out) { err = w + ": bad arguments (1 to 3 sinks)"; return -1; }
    for (int i = 0; i < S.n; ++i) {
        S.out[3 * i] = S.out[3 * i + 1] = S.out[3 * i + 2] = 0;
        if (S.seconds) S.seconds[2 * i] = S.seconds[2 * i + 1] = 0;
    }
    for (int i = 0; i < S.n; ++i) {
        if (!S.tables[i]) { err = w + ": bad arguments (a sink without a table)"; return -1; }
        if (!bincount_mask_ok(S.masks[i])) { err = w + ": the mask of sink " + std::to_string(i) + " is " + std::to_string(S.masks[i]) + "; it must be 1 to 7, a bit per bin code"; return -1; }
    }
    if (!like) like = S.tables[0];
    for (int i = 0; i < S.n; ++i) {
        Table &T = *S.tables[i];
        for (int q = 0; q < n_keep; ++q)
            if (keep && keep[q] == &T) { err = w + ": sink " + std::to_string(i) + " is one of the binning's own tables (mat or pat); a sink is a table of its own"; return -1; }
        for (int j = 0; j < i; ++j)
            if (S.tables[j] == &T) { err = w + ": sinks " + std::to_string(j) + " and " + std::to_string(i) + " are the same table"; return -1; }
        if (T.k != like->k) { err = w + ": the tables have different k (" + std::to_string(like->k) + ", sink " + std::to_string(i) + " " + std::to_string(T.k) + ")"; return -1; }
        if (T.device != like->device) { err = w + ": the tables are on different devices"; return -1; }
        if (T.d.nshard > 1) { err = w + ": sink " + std::to_string(i) + " must be a whole table, not an attached owner-sharded one"; return -1; }
    }
    return 0;
}

int check_batch(int64_t n_reads, const int64_t *offsets, const uint8_t *codes, std::string &err) {
    const std::string w(BC_WHAT);
    switch (bincount_check(n_reads, offsets, codes)) {
    case BC_BAD_ARGS: err = w + ": bad arguments"; return -1;
    case BC_BAD_OFFSETS: err = w + ": offsets must not decrease"; return -1;
    case BC_BAD_CODE: err = w + ": a bin code is not 0, 1 or 2"; return -1;
    case BC_TOO_LARGE: err = w + ": more than 2^31-1 reads or 2^43 text bytes in one call"; return -1;
    default: return 0;
    }
}

// one sink: its list, then gather and count piece by piece.  The text is complete in HBM (the caller has waited for whatever wrote it)
int count_sink(Table &T, uint32_t mask, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, const uint8_t *codes, uint64_t piece, uint64_t out[3], double *seconds,
               std::string &err) {
    SinkList L;
    sink_list(n_reads, offsets, codes, mask, L);
    out[0] = L.reads;
    out[1] = L.bases;
    out[2] = 0;
    if (!L.reads) return 0;
    const uint64_t most = largest_piece(L.dst, piece);
    if (piece_blocks(most) > 0x7FFFFFFFull) { err = std::string(BC_WHAT) + ": a read is too long for one piece"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    hipStream_t st = T.stream;
    const int W = Table::WS_BINCOUNT;
    int64_t *d_src = (int64_t *)T.workspace(W + 1, L.src.size() * sizeof(int64_t), err);
    uint64_t *d_dst = (uint64_t *)T.workspace(W + 2, L.dst.size() * sizeof(uint64_t), err);
    uint8_t *d_out = (uint8_t *)T.workspace(W + 3, piece_room(most), err);
    if (!d_src || !d_dst || !d_out) return -1;
    HIPCHK(hipMemcpyAsync(d_src, L.src.data(), L.src.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_dst, L.dst.data(), L.dst.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    Events ev;
    if (ev.create(err)) return -1;
    if (T.read_stats(err)) return -1;                   // (waits: the lists are up)
    const uint64_t occ_before = T.h_stats[ST_OCCURRENCES];
    double gather = 0, counting = 0;
    for (uint64_t j0 = 0; j0 < L.reads;) {
        const uint64_t j1 = piece_end(L.dst, j0, piece), bytes = L.dst[j1] - L.dst[j0];
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(reads_gather_kernel, dim3((unsigned)piece_blocks(bytes)), dim3(BC_THREADS), 0, st, d_text, d_src, d_dst, j0, j1, piece_groups(bytes), d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = T.count_device(d_out, bytes, err);      // (returns when the piece is in the table: d_out is free again)
        if (rc) return rc;
        counting += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (ev.add_seconds(gather, err)) return -1;
        j0 = j1;
    }
    if (T.read_stats(err)) return -1;
    out[2] = T.h_stats[ST_OCCURRENCES] - occ_before;
    if (seconds) { seconds[0] = gather; seconds[1] = counting; }
    return 0;
}

int count_sinks(const BinSinks &S, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, const uint8_t *codes, std::string &err) {
    uint64_t piece = 0;
    if (piece_bytes(piece, err)) return -1;
    for (int i = 0; i < S.n; ++i) {
        const int rc = count_sink(*S.tables[i], S.masks[i], n_reads, d_text, offsets, codes, piece, S.out + 3 * i, S.seconds ? S.seconds + 2 * i : nullptr, err);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

int count_binned_device(const BinSinks &S, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, const uint8_t *codes, Table *const *keep, int n_keep, std::string &err) {
    if (check_sinks(S, nullptr, keep, n_keep, err) || check_batch(n_reads, offsets, codes, err)) return -1;
    if (n_reads == 0) return 0;
    if (offsets[n_reads] > offsets[0] && !d_text) { err = std::string(BC_WHAT) + ": null text"; return -1; }
    return count_sinks(S, n_reads, d_text, offsets, codes, err);
}

int count_binned_host(const BinSinks &S, int64_t n_reads, const char *text, const int64_t *offsets, const uint8_t *codes, std::string &err) {
    if (check_sinks(S, nullptr, nullptr, 0, err) || check_batch(n_reads, offsets, codes, err)) return -1;
    if (n_reads == 0) return 0;
    const int64_t L = offsets[n_reads] - offsets[0];
    if (L > 0 && !text) { err = std::string(BC_WHAT) + ": null text"; return -1; }
    Table &T = *S.tables[0];
    HIPCHK(hipSetDevice(T.device));
    uint8_t *room = (uint8_t *)T.workspace(Table::WS_BINCOUNT, (size_t)L + 15 + 16, err);
    if (!room) return -1;
    const char *from = text + offsets[0];
    uint8_t *up = room + ((uintptr_t)from & 15u);       // (the kernel takes any alignment; the tests reach every one through the host pointer)
    if (L) HIPCHK(hipMemcpyAsync(up, from, (size_t)L, hipMemcpyHostToDevice, T.stream));
    HIPCHK(jk_stream_wait(T.stream));                   // (the other sinks' streams read it too)
    return count_sinks(S, n_reads, up - offsets[0], offsets, codes, err);
}

int read_text_count(Table &M, Table *P, int64_t n_records, const uint8_t *codes, const BinSinks &S, std::string &err) {
    const std::string w(BC_WHAT);
    Table *const keep[2] = {&M, P};
    if (check_sinks(S, &M, keep, 2, err)) return -1;
    if (M.text_records < 0) { err = w + ": no read-text call has left anything to count"; return -1; }
    if (n_records != M.text_records) { err = w + ": n_records is not what the read-text call returned"; return -1; }
    if (n_records == 0) return 0;
    HIPCHK(hipSetDevice(M.device));
    const int W = Table::WS_READTEXT;
    std::vector<int64_t> offs((size_t)n_records + 1);
    HIPCHK(hipMemcpyAsync(offs.data(), M.ws[W + 8].p, offs.size() * sizeof(int64_t), hipMemcpyDeviceToHost, M.stream));
    HIPCHK(jk_stream_wait(M.stream));                   // (and the packed sequences are complete: the sinks' streams read them)
    if (check_batch(n_records, offs.data(), codes, err)) return -1;
    if (offs[0] != 0 || offs[(size_t)n_records] != M.text_seq_bytes) { err = w + ": the workspace's offsets are not the read-text call's"; return -1; }
    return count_sinks(S, n_records, (const uint8_t *)M.ws[W + 6].p, offs.data(), codes, err);
}

}  // namespace jk
