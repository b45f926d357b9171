// copies.hip -- copy-number scan: every window of every sequence looked up in the reads' table R and in the assembly's table A,
// classified by the copy number the reads support against the copies the assembly holds, as per-sequence counters and the maximal
// runs of each class (semantics: include/jasper_hip.h, jasper_copy_report).
//
// An extension the reference has no counterpart for.  It is the dense scan of report.hip joined with the second table of
// spectra.hip: the spectrum says how many distinct k-mers are collapsed or duplicated, this says where on the contigs they are.
//
//   copies_scan_kernel    report_scan_kernel's tile: RP_TILE windows of ONE sequence per workgroup iteration, thread t owns the 16
//                         windows that end at origin + 16t .., stage16 staging with the 64-base halo, rolling forward and reverse
//                         k-mers.  Per window ONE mix (the hash does not depend on a table's size) and TWO probes: R through
//                         read_slots (the owner's shard when R is attached), A whole.  The home-slot loads of a batch of four windows
//                         are in flight before any is resolved; A's four loads go out after R's four are resolved (CP_A_EARLY: with
//                         them -- DESIGN 4.5 has both measurements).  Both counts stay in LDS (2 x 16 KB) with a 64-bit sum per
//                         group of 16; a thread's windows are two 16-bit class masks (excess / deficit).  A run starts where a class
//                         bit follows a window that does not have that class (clear, the other class, the thread before's last
//                         window) or at the tile's first window, and every start walks its run through its class's masks -- whole
//                         groups by their stored sums -- to the run's or the tile's end.  The tile's PARTIAL runs go to a list (one
//                         cursor add per tile) with the class of the tile's first and last window; five adds per tile into the
//                         per-sequence counters.  Nothing per window leaves the CU.
//   copies_heads_kernel   one workgroup: a partial run is the HEAD of a final run unless it continues the last partial run of the
//                         tile before it (same sequence, the same non-zero class on both sides of the seam); exclusive sum of heads.
//   copies_stitch_kernel  one wave per tile: each head is copied to its final place; the head that is open at its tile's end first
//                         absorbs the continuing partial runs OF ITS KIND of the tiles after it.
//
// The class of a window needs e = (2c + peak) div (2 peak) only in comparison with a; with P = peak * a (< 2^64):
//   e > a  <=>  (2c + peak) / (2 peak) >= a + 1  <=>  2c >= 2P + peak        e < a  <=>  (2c + peak) / (2 peak) < a  <=>  2c + peak < 2P
// and 2c + peak < 2^34, so P >= 2^33 decides both without forming 2P: no 64-bit division per window, the same classes.
//
// The list of partial runs starts at windows / 64 + 64K entries, as the report's; a scan that needed more has counted how many and
// is repeated once with exactly that room.
#include "copies.hpp"
#include <algorithm>
#include <cstring>

#ifndef CP_A_EARLY
#define CP_A_EARLY 0
#endif
#ifndef CP_BATCH_UNROLL
#define CP_BATCH_UNROLL 1      // 1: the four batches of a thread as a loop, 4: unrolled (registers against occupancy)
#endif
#define CP_STR_(x) #x
#define CP_PRAGMA_UNROLL(n) _Pragma(CP_STR_(unroll n))

namespace jk {

#define HIPCHK(x)                                                                     \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            err = std::string(#x) + ": " + hipGetErrorString(e_);                     \
            return -1;                                                                \
        }                                                                             \
    } while (0)

struct CpTile { uint32_t seq, idx; };                                    // tile idx (windows idx * RP_TILE ..) of sequence seq
struct CpTileOut { unsigned long long base; uint32_t nruns, ends; };     // its partial runs: part[base .. base + nruns); ends = first class | last class << 2
enum { CC_CURSOR = 0, CC_HEADS = 1, CC_WORDS = 4 };                      // control words: partial runs wanted, final runs
enum { CP_NCOUNT = 5 };                                                  // device counters per sequence: valid, excess, deficit, sum_reads, sum_asm

__device__ __forceinline__ uint32_t cp_first(uint32_t ends) { return ends & 3u; }
__device__ __forceinline__ uint32_t cp_last(uint32_t ends) { return (ends >> 2) & 3u; }

__device__ __forceinline__ uint32_t cp_incl_scan32(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t cp_sum32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long cp_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(RP_THREADS) void copies_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const CpTile *__restrict__ tiles,
                                                                 uint64_t ntiles, TableDev R, TableDev A, uint32_t thre, uint32_t peak,
                                                                 unsigned long long *__restrict__ counts, CpTileOut *__restrict__ tout, CopyRun *__restrict__ part,
                                                                 unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_c[RP_TILE];                   // count in R of window w0 + i (0 where there is no k-mer)
    __shared__ uint32_t s_a[RP_TILE];                   // ... in A
    __shared__ uint32_t s_ex[RP_THREADS];               // bit j of [g]: window w0 + 16g + j is `excess`
    __shared__ uint32_t s_de[RP_THREADS];               // ... is `deficit`
    __shared__ unsigned long long s_gc[RP_THREADS];     // sum of s_c over group g
    __shared__ unsigned long long s_ga[RP_THREADS];     // ... of s_a
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot[3];                       // valid, excess, deficit windows of the tile
    __shared__ unsigned long long s_sum[2];             // sums of c and of a over the tile's valid windows
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k = R.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const CpTile D = tiles[tile];
        const int64_t o0 = offs[D.seq];
        const int64_t n = offs[D.seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        const int64_t w0 = (int64_t)D.idx * RP_TILE;    // the tile's first window
        const int64_t origin = w0 + k - 1;              // ... ends here
        if (t < 3) s_tot[t] = 0;
        if (t < 2) s_sum[t] = 0ull;
        uint32_t c, iv;
        stage16(txt, origin + (int64_t)t * RP_GROUP, n, c, iv);
        s_code[t + RP_HALO] = c;
        s_inv[t + RP_HALO] = iv;
        if (t < RP_HALO) {
            uint32_t hc, hiv;
            stage16(txt, origin - (int64_t)(RP_HALO - t) * RP_GROUP, n, hc, hiv);
            s_code[t] = hc;
            s_inv[t] = hiv;
        }
        __syncthreads();
        const uint32_t w4 = s_code[t], w3 = s_code[t + 1], w2 = s_code[t + 2], w1 = s_code[t + 3];
        const uint64_t ivprev = ((uint64_t)s_inv[t] << 48) | ((uint64_t)s_inv[t + 1] << 32) | ((uint64_t)s_inv[t + 2] << 16) | (uint64_t)s_inv[t + 3];
        u128 fwd = band(mk(((uint64_t)w4 << 32) | w3, ((uint64_t)w2 << 32) | w1), kmask);
        u128 rc = revcomp(fwd, k);
        int run = ivprev ? (int)__builtin_ctzll(ivprev) : 64;
        const int64_t e0 = origin + (int64_t)t * RP_GROUP;
        uint32_t vm = 0, em = 0, dm = 0;
        unsigned long long gc = 0, ga = 0;
        CP_PRAGMA_UNROLL(CP_BATCH_UNROLL)
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 er[4], ea[4];
            uint32_t cr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const uint32_t cj = (c >> (30 - 2 * j)) & 3u;
                const bool bad = (iv >> (15 - j)) & 1u;
                fwd = band(bor(shl(fwd, 2), mk(0, cj)), kmask);
                rc = bor(shr(rc, 2), shl(mk(0, 3u - cj), 2 * (k - 1)));
                run = bad ? 0 : run + 1;
                ok[u] = run >= k && e0 + j < n;
                hs[u] = mix(lt(rc, fwd) ? rc : fwd, R.B);
                er[u] = make_ulonglong2(0ull, 0ull);
                ea[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) {
                    er[u] = *reinterpret_cast<const ulonglong2 *>(read_slots(R, hs[u]) + 2 * home_of(hs[u], R.B, R.s));
#if CP_A_EARLY
                    ea[u] = *reinterpret_cast<const ulonglong2 *>(A.slots + 2 * home_of(hs[u], A.B, A.s));
#endif
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                cr[u] = ok[u] ? clamp32(table_get_prefetched(R, hs[u], er[u])) : 0u;
#if !CP_A_EARLY
                if (ok[u]) ea[u] = *reinterpret_cast<const ulonglong2 *>(A.slots + 2 * home_of(hs[u], A.B, A.s));
#endif
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const uint32_t ca = ok[u] ? clamp32(table_get_prefetched(A, hs[u], ea[u])) : 0u;
                const unsigned long long P = (unsigned long long)peak * ca, c2 = 2ull * cr[u];
                const bool solid = ok[u] && cr[u] >= thre;
                const bool big = P >= (1ull << 33);
                const bool ex = solid && !big && 2ull * P + peak <= c2;
                const bool de = solid && (big || c2 + peak < 2ull * P);
                s_c[t * RP_GROUP + j] = cr[u];
                s_a[t * RP_GROUP + j] = ca;
                vm |= (ok[u] ? 1u : 0u) << j;
                em |= (ex ? 1u : 0u) << j;
                dm |= (de ? 1u : 0u) << j;
                gc += cr[u];
                ga += ca;
            }
        }
        s_ex[t] = em;
        s_de[t] = dm;
        s_gc[t] = gc;
        s_ga[t] = ga;
        {
            const uint32_t cv = cp_sum32(__popc(vm)), ce = cp_sum32(__popc(em)), cd = cp_sum32(__popc(dm));
            const unsigned long long sc = cp_sum64(gc), sa = cp_sum64(ga);
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], ce);
                atomicAdd(&s_tot[2], cd);
                atomicAdd(&s_sum[0], sc);
                atomicAdd(&s_sum[1], sa);
            }
        }
        __syncthreads();
        // where my runs start: a class bit after a window that does not have that class (the tile's first window starts one anyway)
        const uint32_t pe = t > 0 ? (s_ex[t - 1] >> 15) & 1u : 0u, pd = t > 0 ? (s_de[t - 1] >> 15) & 1u : 0u;
        const uint32_t se = em & ~((em << 1) | pe) & 0xFFFFu, sd = dm & ~((dm << 1) | pd) & 0xFFFFu;
        const uint32_t startmask = se | sd;             // (no window has both classes)
        const uint32_t ns = __popc(startmask);
        const uint32_t incl = cp_incl_scan32(ns);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RP_THREADS / 64; ++w) {
            woff += w < wave ? s_wsum[w] : 0u;
            total += s_wsum[w];
        }
        if (t == 0) {
            const unsigned long long b = total ? atomicAdd(&ctl[CC_CURSOR], (unsigned long long)total) : 0ull;
            s_base = b;
            CpTileOut O;
            O.base = b;
            O.nruns = total;
            const uint32_t e0m = s_ex[0], d0m = s_de[0], eLm = s_ex[RP_THREADS - 1], dLm = s_de[RP_THREADS - 1];
            const uint32_t first = (e0m & 1u) ? CP_EXCESS : (d0m & 1u) ? CP_DEFICIT : CP_NONE;
            const uint32_t last = ((eLm >> 15) & 1u) ? CP_EXCESS : ((dLm >> 15) & 1u) ? CP_DEFICIT : CP_NONE;
            O.ends = first | (last << 2);
            tout[tile] = O;
        }
        if (t < 3 && s_tot[t]) atomicAdd(&counts[(unsigned long long)CP_NCOUNT * D.seq + t], (unsigned long long)s_tot[t]);
        if (t >= 3 && t < 5 && s_sum[t - 3]) atomicAdd(&counts[(unsigned long long)CP_NCOUNT * D.seq + t], s_sum[t - 3]);
        __syncthreads();
        const unsigned long long base = s_base;
        if (base + total <= cap) {
            uint32_t sm = startmask;
            unsigned long long at = base + woff + incl - ns;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                const bool isex = (se >> b0) & 1u;
                const uint32_t *__restrict__ M = isex ? s_ex : s_de;
                int pos = t * RP_GROUP + b0;
                uint64_t nk = 0, sr = 0, sa = 0;
                while (pos < RP_TILE) {
                    const int g = pos >> 4, b = pos & 15;
                    const uint32_t U = M[g] >> b;
                    const int len = __builtin_ctz(~U);            // (bits 16.. of U are clear: len <= 16 - b)
                    if (len == 0) break;
                    if (len == RP_GROUP) {
                        sr += s_gc[g];
                        sa += s_ga[g];
                    } else {
                        for (int j = 0; j < len; ++j) {
                            sr += s_c[pos + j];
                            sa += s_a[pos + j];
                        }
                    }
                    nk += len;
                    pos += len;
                    if (b + len < RP_GROUP) break;
                }
                CopyRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = nk;
                r.sum_reads = sr;
                r.sum_asm = sa;
                r.seq = D.seq;
                r.kind = isex ? CP_EXCESS : CP_DEFICIT;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

// 1 if the first partial run of tile i continues the last one of tile i - 1: the same class on both sides of the seam
__device__ __forceinline__ uint32_t cp_cont(const CpTile *__restrict__ tiles, const CpTileOut *__restrict__ tout, uint64_t i) {
    if (i == 0 || tiles[i].idx == 0) return 0u;         // (idx > 0: tile i - 1 is the tile before it in the same sequence)
    const uint32_t f = cp_first(tout[i].ends);
    return f != CP_NONE && f == cp_last(tout[i - 1].ends) ? 1u : 0u;
}

constexpr int CH_THREADS = 1024;
__global__ __launch_bounds__(CH_THREADS) void copies_heads_kernel(const CpTile *__restrict__ tiles, const CpTileOut *__restrict__ tout, uint64_t ntiles,
                                                                  unsigned long long *__restrict__ head_base, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_w[CH_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t per = (ntiles + CH_THREADS - 1) / CH_THREADS;
    const uint64_t lo = (uint64_t)t * per < ntiles ? (uint64_t)t * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    unsigned long long sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += tout[i].nruns - cp_cont(tiles, tout, i);
    unsigned long long incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long at = incl - sum;
    for (int w = 0; w < wave; ++w) at += s_w[w];
    for (uint64_t i = lo; i < hi; ++i) {
        head_base[i] = at;
        at += tout[i].nruns - cp_cont(tiles, tout, i);
    }
    if (t == CH_THREADS - 1) ctl[CC_HEADS] = at;
}

__global__ __launch_bounds__(256) void copies_stitch_kernel(const CpTile *__restrict__ tiles, const CpTileOut *__restrict__ tout,
                                                            const unsigned long long *__restrict__ head_base, uint64_t ntiles, const CopyRun *__restrict__ part,
                                                            CopyRun *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ntiles; i += nwv) {
        const CpTileOut O = tout[i];
        const uint32_t cont = cp_cont(tiles, tout, i);
        for (uint32_t j = lane + cont; j < O.nruns; j += 64) {
            CopyRun r = part[O.base + j];
            if (j == O.nruns - 1 && cp_last(O.ends) != CP_NONE) {      // (the run that holds the tile's last window is its last one: r.kind is that class)
                for (uint64_t q = i + 1; q < ntiles && tiles[q].idx != 0; ++q) {
                    const CpTileOut Q = tout[q];
                    if (cp_first(Q.ends) != r.kind) break;
                    const CopyRun p = part[Q.base];
                    r.n_kmers += p.n_kmers;
                    r.sum_reads += p.sum_reads;
                    r.sum_asm += p.sum_asm;
                    if (Q.nruns != 1 || cp_last(Q.ends) != r.kind) break;      // that run ends inside tile q
                }
            }
            out[head_base[i] + j - cont] = r;
        }
    }
}

namespace {
struct Events {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
int check_pair(Table &R, Table &A, uint32_t peak, std::string &err) {
    if (&R == &A) { err = "copy report: the read table and the assembly table are the same table"; return -1; }
    if (R.k != A.k) { err = "copy report: the tables have different k (" + std::to_string(R.k) + " and " + std::to_string(A.k) + ")"; return -1; }
    if (R.device != A.device) { err = "copy report: the tables are on different devices"; return -1; }
    if (A.d.nshard > 1) { err = "copy report: the assembly table must be a whole table, not an attached owner-sharded one"; return -1; }
    if (peak < 1) { err = "copy report: peak must be at least 1"; return -1; }
    return 0;
}
}  // namespace

int copies_report_device(Table &R, Table &A, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak, CopyOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "copy report: bad arguments"; return -1; }
    if (check_pair(R, A, peak, err)) return -1;
    HIPCHK(hipSetDevice(R.device));
    // a logically empty table holds garbage until it is zeroed: both tables are probed
    if (A.materialize(err) || R.materialize(err)) return -1;
    const int k = R.k;
    out.counts.assign((size_t)n_seqs * 6, 0);
    out.runs.clear();
    out.seconds = 0;
    out.retried = 0;
    std::vector<CpTile> tiles;
    uint64_t windows = 0;
    for (int i = 0; i < n_seqs; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0) { err = "copy report: offsets must not decrease"; return -1; }
        const int64_t n = offsets[i + 1] - offsets[i];
        const uint64_t w = n >= k ? (uint64_t)(n - k + 1) : 0;
        out.counts[6 * (size_t)i] = w;
        windows += w;
        const uint64_t nt = (w + RP_TILE - 1) / RP_TILE;
        if (nt > 0xFFFFFFFFull) { err = "copy report: sequence too long"; return -1; }
        for (uint64_t q = 0; q < nt; ++q) tiles.push_back(CpTile{(uint32_t)i, (uint32_t)q});
    }
    const uint64_t ntiles = tiles.size();
    if (ntiles == 0) return 0;
    if (!d_text) { err = "copy report: null text"; return -1; }
    hipStream_t st = R.stream;
    const int W = Table::WS_COPIES;
    int64_t *d_offs = (int64_t *)R.workspace(W + 1, ((size_t)n_seqs + 1) * sizeof(int64_t), err);
    CpTile *d_tiles = (CpTile *)R.workspace(W + 2, ntiles * sizeof(CpTile), err);
    CpTileOut *d_tout = (CpTileOut *)R.workspace(W + 3, ntiles * sizeof(CpTileOut), err);
    unsigned long long *d_head = (unsigned long long *)R.workspace(W + 4, ntiles * sizeof(unsigned long long), err);
    const size_t cnt_words = (size_t)n_seqs * CP_NCOUNT + CC_WORDS;
    unsigned long long *d_cnt = (unsigned long long *)R.workspace(W + 5, cnt_words * sizeof(unsigned long long), err);
    if (!d_offs || !d_tiles || !d_tout || !d_head || !d_cnt) return -1;
    unsigned long long *d_ctl = d_cnt + (size_t)n_seqs * CP_NCOUNT;
    Events ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(ev.e[4], A.stream));        // whatever A's stream still does to A comes first
    HIPCHK(hipStreamWaitEvent(st, ev.e[4], 0));
    HIPCHK(hipMemcpyAsync(d_offs, offsets, ((size_t)n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), ntiles * sizeof(CpTile), hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 256 * 8);
    unsigned long long cap = windows / 64 + 65536, ctl[CC_WORDS] = {0, 0, 0, 0};
    CopyRun *d_part = nullptr;
    for (int attempt = 0;; ++attempt) {
        d_part = (CopyRun *)R.workspace(W + 6, cap * sizeof(CopyRun), err);
        if (!d_part) return -1;
        HIPCHK(hipMemsetAsync(d_cnt, 0, cnt_words * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(copies_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, d_offs, d_tiles, ntiles, R.d, A.d, thre, peak, d_cnt, d_tout, d_part, cap,
                           d_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        out.seconds += ms * 1e-3;
        if (ctl[CC_CURSOR] <= cap) break;
        if (attempt) { err = "copy report: the number of partial runs changed between two scans"; return -1; }
        cap = ctl[CC_CURSOR];            // the scan counted what it could not write: exactly this much room is needed
        out.retried = 1;
    }
    const uint64_t nparts = ctl[CC_CURSOR];
    std::vector<unsigned long long> cnt((size_t)n_seqs * CP_NCOUNT);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (nparts) {
        CopyRun *d_out = (CopyRun *)R.workspace(W + 7, nparts * sizeof(CopyRun), err);
        if (!d_out) return -1;
        HIPCHK(hipEventRecord(ev.e[2], st));
        hipLaunchKernelGGL(copies_heads_kernel, dim3(1), dim3(CH_THREADS), 0, st, d_tiles, d_tout, ntiles, d_head, d_ctl);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(copies_stitch_kernel, dim3((unsigned)std::min<uint64_t>((ntiles + 3) / 4, 256 * 16)), dim3(256), 0, st, d_tiles, d_tout, d_head, ntiles, d_part,
                           d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[3], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
        out.seconds += ms * 1e-3;
        const uint64_t nruns = ctl[CC_HEADS];
        if (nruns > nparts) { err = "copy report: more runs than partial runs"; return -1; }
        out.runs.resize(nruns);
        if (nruns) HIPCHK(hipMemcpyAsync(out.runs.data(), d_out, nruns * sizeof(CopyRun), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(jk_stream_wait(st));
    for (int i = 0; i < n_seqs; ++i)
        for (int c = 0; c < CP_NCOUNT; ++c) out.counts[6 * (size_t)i + 1 + c] = cnt[CP_NCOUNT * (size_t)i + c];
    return 0;
}

int copies_report_host(Table &R, Table &A, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak, CopyOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "copy report: bad arguments"; return -1; }
    if (check_pair(R, A, peak, err)) return -1;
    HIPCHK(hipSetDevice(R.device));
    std::vector<int64_t> offs((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        if (lens[i] < 0 || (lens[i] && !seqs[i])) { err = "copy report: bad sequence"; return -1; }
        offs[i + 1] = offs[i] + lens[i];
    }
    const size_t total = (size_t)offs[n_seqs];
    uint8_t *d_text = (uint8_t *)R.workspace(Table::WS_COPIES, total + 16, err);
    if (!d_text) return -1;
    if (n_seqs == 1) {
        if (total) HIPCHK(hipMemcpyAsync(d_text, seqs[0], total, hipMemcpyHostToDevice, R.stream));
        return copies_report_device(R, A, n_seqs, d_text, offs.data(), thre, peak, out, err);
    }
    std::vector<char> all(total);      // one copy for many short sequences; it lives until the scan's last wait has returned
    for (int i = 0; i < n_seqs; ++i)
        if (lens[i]) memcpy(all.data() + offs[i], seqs[i], (size_t)lens[i]);
    if (total) HIPCHK(hipMemcpyAsync(d_text, all.data(), total, hipMemcpyHostToDevice, R.stream));
    return copies_report_device(R, A, n_seqs, d_text, offs.data(), thre, peak, out, err);
}

}  // namespace jk
