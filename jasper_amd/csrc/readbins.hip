// readbins.hip -- trio read binning: every window of every read of a packed batch looked up in the mother's table M and the father's
// table P, and per read the number of maternal-only and of paternal-only windows (semantics: include/jasper_hip.h, jasper_read_bins).
//
// An extension the reference has no counterpart for.  The probes are the hap-mer scan's without a child table (hapmers.hip); what differs
// is the text: millions of reads of ~150 bases back to back instead of a few long contigs.  A tile of one SEQUENCE would be 3 % full, so
// the tiles here are cut over the packed TEXT: the whole batch is the one sequence tile_prologue stages, a thread owns 16 consecutive
// bytes of it, and where the reads begin comes from a bit per text byte.
//
//   read_starts_kernel  the pre-pass: offsets[i] scattered into one start bit per text byte (an atomic OR per read; empty reads set the
//                       bit of the read after them once more).
//   read_bins_kernel    tile_prologue's staging with the tile's start bits beside the invalid masks (s_st: the same layout, first byte in
//                       bit 15), so a thread's rolling state before its first window ends at the last read start of the 64 bytes
//                       before it; roll_window with `run` set to 0 at a start bit before that byte is added, so no window spans two
//                       reads; ONE mix per window and the home-slot loads of a batch of four windows into M and P in flight before any is
//                       resolved, as hapmer_scan_kernel has them.  A thread's result is two 16-bit masks.  Markers are a few per cent of
//                       the windows, so the read a marker belongs to is found on demand: a thread cuts its 16 windows at its start bits,
//                       and for each piece that holds a marker searches the offsets for the piece's read -- between the reads of the
//                       tile's first and last byte, which two threads of the tile have searched for while the text was staged -- and
//                       adds the piece's two sums to that read's counters: one atomic add per thread, read and class.
// The host stage orders the two tables (settle), uploads the offsets, zeroes counters and bits, and times the two kernels by HIP events:
// read_bins_core, which the read-text path (readtext.hip) calls with offsets its own kernels have left in HBM.
#include "readbins.hpp"
#include "hapmers.hpp"
#include "scan_tile.hpp"

namespace jk {

constexpr int RS_THREADS = 256;

// bits: bit (p & 31) of word p >> 5 = a read begins at byte p of the stream (p counted from offs[0]); zeroed before
__global__ __launch_bounds__(RS_THREADS) void read_starts_kernel(const int64_t *__restrict__ offs, int64_t n_reads, uint32_t *__restrict__ bits) {
    const int64_t base = offs[0], end = offs[n_reads];
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n_reads; i += stride) {
        const int64_t o = offs[i];
        if (o < end) atomicOr(&bits[(o - base) >> 5], 1u << ((o - base) & 31));      // (empty reads at the very end begin no byte)
    }
}

// the start bits of the 16 stream bytes pos .. pos + 15, bit j = byte pos + j; bytes outside the stream [0, L) begin no read.  The bit
// array holds one word more than the stream has bits for.
__device__ __forceinline__ uint32_t start16(const uint32_t *__restrict__ bits, int64_t pos, int64_t L) {
    if (pos <= -RP_GROUP || pos >= L) return 0u;
    const int64_t q = pos < 0 ? 0 : pos;
    const uint64_t w = (uint64_t)bits[q >> 5] | ((uint64_t)bits[(q >> 5) + 1] << 32);
    const uint32_t v = (uint32_t)(w >> (q & 31)) & 0xFFFFu;
    return pos < 0 ? (v << (int)(-pos)) & 0xFFFFu : v;
}
__device__ __forceinline__ uint32_t first_in_bit15(uint32_t m16) { return __brev(m16) >> 16; }      // stage16's layout of its invalid mask

// the read that holds text byte pos: the LAST i of lo .. hi with offs[i] <= pos (empty reads before it share its offset).  offs[lo] <= pos.
__device__ __forceinline__ int read_of(const int64_t *__restrict__ offs, int lo, int hi, int64_t pos) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (offs[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// offs: the n_reads + 1 offsets and after them the stream as tile_prologue's one sequence, {offs[0], offs[n_reads]}
__global__ __launch_bounds__(RP_THREADS) void read_bins_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, int64_t n_reads,
                                                               const uint32_t *__restrict__ bits, uint64_t ntiles, TableDev M, TableDev P, uint32_t thre_mat, uint32_t thre_pat,
                                                               uint32_t *__restrict__ mat, uint32_t *__restrict__ pat) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_st[RP_THREADS + RP_HALO];     // start bits, laid out as s_inv
    __shared__ int s_rng[2];                            // the reads of the tile's first and last byte
    static_assert(RP_HALO == 4 && RP_THREADS > 64, "the four groups before a thread's; the two searches run in two waves");
    const int t = threadIdx.x;
    const int k = M.k;
    const u128 kmask = maskbits(2 * k);
    const int64_t *__restrict__ span = offs + n_reads + 1;
    const int64_t base = span[0], L = span[1] - base;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = {0u, (uint32_t)tile};
        const int64_t origin = (int64_t)tile * RP_TILE + k - 1;      // the tile's first window ends here: origin < L
        const uint32_t sj = start16(bits, origin + (int64_t)t * RP_GROUP, L);
        const uint32_t st = first_in_bit15(sj);
        s_st[t + RP_HALO] = st;
        if (t < RP_HALO) s_st[t] = first_in_bit15(start16(bits, origin - (int64_t)(RP_HALO - t) * RP_GROUP, L));
        if (t == 0) s_rng[0] = read_of(offs, 0, (int)(n_reads - 1), base + origin);
        if (t == 64) s_rng[1] = read_of(offs, 0, (int)(n_reads - 1), base + (origin + RP_TILE < L ? origin + RP_TILE : L) - 1);
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, span, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);      // (its barrier is s_st's and s_rng's too)
        {
            const uint32_t *ps = s_st + t;              // the four groups before mine: byte e0 - 1 is bit 0
            const uint64_t stprev = ((uint64_t)ps[0] << 48) | ((uint64_t)ps[1] << 32) | ((uint64_t)ps[2] << 16) | (uint64_t)ps[3];
            if (stprev) run = min(run, (int)__builtin_ctzll(stprev) + 1);      // the bases in a row that end before e0 begin at that start at the earliest
        }
        uint32_t mm = 0, pm = 0;
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 em[4], ep[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                if ((st >> (15 - j)) & 1u) run = 0;     // a read begins at this byte: nothing before it is in its windows
                ok[u] = roll_window(c, iv, j, k, kmask, M.B, e0, n, fwd, rc, run, hs[u]);
                em[u] = make_ulonglong2(0ull, 0ull);
                ep[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) {                            // (M and P are whole tables: their own slot arrays)
                    em[u] = *reinterpret_cast<const ulonglong2 *>(M.slots + 2 * home_of(hs[u], M.B, M.s));
                    ep[u] = *reinterpret_cast<const ulonglong2 *>(P.slots + 2 * home_of(hs[u], P.B, P.s));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const uint32_t m = ok[u] ? clamp32(table_get_prefetched(M, hs[u], em[u])) : 0u;
                const uint32_t p = ok[u] ? clamp32(table_get_prefetched(P, hs[u], ep[u])) : 0u;
                mm |= (ok[u] && m >= thre_mat && p == 0u ? 1u : 0u) << j;
                pm |= (ok[u] && p >= thre_pat && m == 0u ? 1u : 0u) << j;
            }
        }
        if (mm | pm) {
            // my 16 windows cut where a read begins after the first of them; a piece's windows end in one read
            const uint32_t cuts = sj & 0xFFFEu;
            const int lo = s_rng[0], hi = s_rng[1];
            int a = 0;
            while (a < RP_GROUP) {
                const uint32_t later = cuts & ~((2u << a) - 1u);
                const int b = later ? __builtin_ctz(later) : RP_GROUP;
                const uint32_t piece = ((1u << b) - 1u) & ~((1u << a) - 1u);
                const uint32_t cm = __popc(mm & piece), cp = __popc(pm & piece);
                if (cm | cp) {
                    const int i = read_of(offs, lo, hi, base + e0 + a);
                    if (cm) atomicAdd(&mat[i], cm);
                    if (cp) atomicAdd(&pat[i], cp);
                }
                a = b;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

namespace {
const char *const RB_WHAT = "read bins";

// what both entry points refuse before anything is uploaded; L = the stream's bytes
int check_reads(int64_t n_reads, const void *text, const int64_t *offsets, int k, const uint32_t *out_mat, const uint32_t *out_pat, int64_t &L, std::string &err) {
    const std::string w(RB_WHAT);
    L = 0;
    if (n_reads < 0 || (n_reads && (!offsets || !out_mat || !out_pat))) { err = w + ": bad arguments"; return -1; }
    if (n_reads > RB_MAX_READS) { err = w + ": more than 2^31-1 reads in one call"; return -1; }
    if (n_reads == 0) return 0;
    if (offsets[0] < 0) { err = w + ": offsets must not decrease"; return -1; }
    for (int64_t i = 0; i < n_reads; ++i) {
        if (offsets[i + 1] < offsets[i]) { err = w + ": offsets must not decrease"; return -1; }
        if (offsets[i + 1] - offsets[i] - k + 1 > RB_MAX_READ_WINDOWS) { err = w + ": a read has more than 2^32-1 windows"; return -1; }
    }
    L = offsets[n_reads] - offsets[0];
    if (L > RB_MAX_TEXT) { err = w + ": more than 2^43 text bytes in one call"; return -1; }
    if (L > 0 && !text) { err = w + ": null text"; return -1; }
    return 0;
}
}  // namespace

// the core: settle, start bits, scan.  The offsets are in HBM already (d_offs_in: n_reads + 1 offsets and the two words of the stream's
// span behind them), or on the host (h_offs, uploaded into the binning's own slot).  L = the stream's bytes; n_reads > 0.  The counters
// stay in WS_READBINS + 1 (*d_cnt_out: mat[n_reads], then pat[n_reads]); ev times the kernels once the stream has been waited for.
int read_bins_core(Table &M, Table &P, int64_t n_reads, const uint8_t *d_text, const int64_t *h_offs, const int64_t *d_offs_in, int64_t L, uint32_t thre_mat, uint32_t thre_pat,
                   Events &ev, uint32_t **d_cnt_out, std::string &err) {
    M.text_records = -1;                                // (the counters of a read-text call are about to be overwritten: readtext.hip)
    const size_t n = (size_t)n_reads;
    const uint64_t ntiles = L >= M.k ? ((uint64_t)(L - M.k + 1) + RP_TILE - 1) / RP_TILE : 0;
    HIPCHK(hipSetDevice(M.device));
    Table *others[1] = {&P};
    Events order;
    if (settle(M, others, 1, order, err)) return -1;
    hipStream_t st = M.stream;
    const size_t bit_words = (size_t)((L + 31) / 32) + 1;
    int64_t *d_offs = h_offs ? (int64_t *)M.workspace(Table::WS_READBINS, (n + 3) * sizeof(int64_t), err) : const_cast<int64_t *>(d_offs_in);
    uint32_t *d_cnt = (uint32_t *)M.workspace(Table::WS_READBINS + 1, 2 * n * sizeof(uint32_t), err);
    uint32_t *d_bits = (uint32_t *)M.workspace(Table::WS_READBINS + 2, bit_words * sizeof(uint32_t), err);
    if (!d_offs || !d_cnt || !d_bits) return -1;
    if (h_offs) {
        const int64_t span[2] = {h_offs[0], h_offs[n]};
        HIPCHK(hipMemcpyAsync(d_offs, h_offs, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_offs + n + 1, span, sizeof span, hipMemcpyHostToDevice, st));
    }
    if (ev.create(err)) return -1;
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(hipMemsetAsync(d_cnt, 0, 2 * n * sizeof(uint32_t), st));
    if (ntiles) {                                       // (no tile: no window anywhere, the counters are zeros)
        HIPCHK(hipMemsetAsync(d_bits, 0, bit_words * sizeof(uint32_t), st));
        hipLaunchKernelGGL(read_starts_kernel, dim3((unsigned)std::min<uint64_t>((n + RS_THREADS - 1) / RS_THREADS, 256 * 8)), dim3(RS_THREADS), 0, st, d_offs, n_reads, d_bits);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(read_bins_kernel, dim3((unsigned)std::min<uint64_t>(ntiles, 256 * 8)), dim3(RP_THREADS), 0, st, d_text, d_offs, n_reads, d_bits, ntiles, M.d, P.d, thre_mat,
                           thre_pat, d_cnt, d_cnt + n);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev.e[1], st));
    *d_cnt_out = d_cnt;
    return 0;
}

int read_bins_device(Table &M, Table &P, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t *out_mat,
                     uint32_t *out_pat, double *seconds, std::string &err) {
    if (seconds) *seconds = 0;
    if (check_trio(RB_WHAT, M, P, nullptr, nullptr, thre_mat, thre_pat, 1, err)) return -1;
    int64_t L;
    if (check_reads(n_reads, d_text, offsets, M.k, out_mat, out_pat, L, err)) return -1;
    if (n_reads == 0) return 0;
    const size_t n = (size_t)n_reads;
    if (L < M.k) {                                      // no window anywhere
        std::fill(out_mat, out_mat + n, 0u);
        std::fill(out_pat, out_pat + n, 0u);
        return 0;
    }
    Events ev;
    uint32_t *d_cnt = nullptr;
    if (read_bins_core(M, P, n_reads, d_text, offsets, nullptr, L, thre_mat, thre_pat, ev, &d_cnt, err)) return -1;
    hipStream_t st = M.stream;
    HIPCHK(hipMemcpyAsync(out_mat, d_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_pat, d_cnt + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) *seconds = s;
    return 0;
}

int read_bins_host(Table &M, Table &P, int64_t n_reads, const char *text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t *out_mat, uint32_t *out_pat,
                   double *seconds, std::string &err) {
    if (seconds) *seconds = 0;
    if (check_trio(RB_WHAT, M, P, nullptr, nullptr, thre_mat, thre_pat, 1, err)) return -1;
    int64_t L;
    if (check_reads(n_reads, text, offsets, M.k, out_mat, out_pat, L, err)) return -1;
    if (n_reads == 0) return 0;
    HIPCHK(hipSetDevice(M.device));
    uint8_t *d_text = (uint8_t *)M.workspace(Table::WS_READBINS + 3, (size_t)L + 16, err);
    if (!d_text) return -1;
    if (L) HIPCHK(hipMemcpyAsync(d_text, text + offsets[0], (size_t)L, hipMemcpyHostToDevice, M.stream));
    std::vector<int64_t> rel((size_t)n_reads + 1);      // the offsets from the first uploaded byte on
    for (size_t i = 0; i < rel.size(); ++i) rel[i] = offsets[i] - offsets[0];
    return read_bins_device(M, P, n_reads, d_text, rel.data(), thre_mat, thre_pat, out_mat, out_pat, seconds, err);
}

}  // namespace jk
