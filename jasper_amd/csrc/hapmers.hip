// hapmers.hip -- trio hap-mer scan and census: every window of every sequence looked up in the mother's table M and the father's table P
// (and, for the windows those two make candidates, in the child's table R), classified as maternal-only or paternal-only, as per-sequence
// counters and the maximal runs of each class; and the same three tables swept slot by slot against the assembly's table A (semantics:
// include/jasper_hip.h, jasper_hapmer_scan and jasper_hapmer_census).
//
// An extension the reference has no counterpart for: the trio half of a k-mer evaluation.  The phase blocks are host work
// (jasper_amd/hapmers.py); what needs the tables happens here.
//
//   hapmer_scan_kernel    the dense scans' tile (scan_tile.hpp).  Per window ONE mix (the hash does not depend on a table's size) and TWO
//                         unconditional probes, M and P, both whole tables; the home-slot loads of a batch of four windows into both are
//                         in flight before any is resolved.  A window whose counts in M and P make it a candidate -- a few per cent of the
//                         windows (6.7 % on the measurement workload) -- is then looked up in R by a plain table_get under that branch (through read_slots:
//                         the owner's shard when R is attached); no load registers are kept for R.  A thread's windows are two 16-bit class
//                         masks (mat / pat) in LDS and nothing else: a run's length follows from the masks, so there are no count arrays
//                         and no group sums, and LDS per workgroup is 4 168 B where the copy scan has 41 048 B.  Run starts and the walk
//                         through the class's masks are the shared run finder (class_starts, tile_ends2, walk_run of scan_tile.hpp)
//                         with nothing to accumulate per piece.  The tile's PARTIAL runs go to a list (one
//                         cursor add per tile) with the class of the tile's first and last window; three adds per tile into the
//                         per-sequence counters.
//   hapmer_census_kernel  a sweep over M's slots in the shape of spectra_reads_kernel: slots whose count is below the threshold are dropped
//                         before any probe, the others probe P with the loads of the batch in flight together, the survivors (P has none)
//                         probe R and then A.  Three counters per thread, summed per wave and per workgroup, three global adds per
//                         workgroup.  Launched twice, the parents swapped.
// A window's rolling step, the heads and stitch kernels that make final runs of the partial ones, and the host stage (settle, run_scan)
// are the shared ones of scan_tile.hpp; the census orders its four tables with the same settle.
#include "hapmers.hpp"
#include "scan_tile.hpp"
#include "spectra.hpp"

#ifndef HM_BATCH_UNROLL
#define HM_BATCH_UNROLL 1      // 1: the four batches of a thread as a loop, 4: unrolled (registers against occupancy)
#endif
#define HM_STR_(x) #x
#define HM_PRAGMA_UNROLL(n) _Pragma(HM_STR_(unroll n))

namespace jk {

enum { HM_NCOUNT = 3 };                                                  // device counters per sequence: valid, mat, pat
enum { HC_WORDS = 6 };                                                   // the census's words: hapmers, found, occurrences of mat, then of pat

__device__ __forceinline__ uint32_t kind_of(HapRun r) { return r.kind; }
__device__ __forceinline__ HapRun absorb(HapRun r, HapRun p) {
    r.n_kmers += p.n_kmers;
    return r;
}

__global__ __launch_bounds__(RP_THREADS) void hapmer_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                                 uint64_t ntiles, TableDev M, TableDev P, TableDev R, int has_child, uint32_t thre_mat, uint32_t thre_pat,
                                                                 uint32_t thre_child, unsigned long long *__restrict__ counts, TileRuns *__restrict__ tout,
                                                                 HapRun *__restrict__ part, unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_ma[RP_THREADS];               // bit j of [g]: window w0 + 16g + j is `mat`
    __shared__ uint32_t s_pa[RP_THREADS];               // ... is `pat`
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot[HM_NCOUNT];               // valid, mat, pat windows of the tile
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const int k = M.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t < HM_NCOUNT) s_tot[t] = 0;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        uint32_t vm = 0, mm = 0, pm = 0;
        HM_PRAGMA_UNROLL(HM_BATCH_UNROLL)
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 em[4], ep[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
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
                bool ma = ok[u] && m >= thre_mat && p == 0u;
                bool pa = ok[u] && p >= thre_pat && m == 0u;
                if (has_child && (ma || pa)) {          // a few per cent of the windows: one dependent lookup, no registers held for it across the batch
                    const bool kept = clamp32(table_get(R, hs[u])) >= thre_child;
                    ma = ma && kept;
                    pa = pa && kept;
                }
                vm |= (ok[u] ? 1u : 0u) << j;
                mm |= (ma ? 1u : 0u) << j;
                pm |= (pa ? 1u : 0u) << j;
            }
        }
        s_ma[t] = mm;
        s_pa[t] = pm;
        {
            const uint32_t cv = wave_sum(__popc(vm)), cm = wave_sum(__popc(mm)), cp = wave_sum(__popc(pm));
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], cm);
                atomicAdd(&s_tot[2], cp);
            }
        }
        __syncthreads();
        // where my runs start: a class bit after a window that does not have that class (the tile's first window starts one anyway)
        const uint32_t sm_ = class_starts(mm, s_ma), sp_ = class_starts(pm, s_pa);
        const uint32_t startmask = sm_ | sp_;           // (no window has both classes)
        const uint32_t ns = __popc(startmask);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, tile_ends2(s_ma, s_pa, HM_MAT, HM_PAT)};
        if (t < HM_NCOUNT && s_tot[t]) atomicAdd(&counts[(unsigned long long)HM_NCOUNT * D.seq + t], (unsigned long long)s_tot[t]);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                const bool ismat = (sm_ >> b0) & 1u;
                HapRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = walk_run(ismat ? s_ma : s_pa, t * RP_GROUP + b0, [](int, int, int, int) {});      // (a run's length is all there is to it)
                r.seq = D.seq;
                r.kind = ismat ? HM_MAT : HM_PAT;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

// Sweep over the slots of M (a whole table): H = its keys with count >= thre that P does not have and (with has_r) R has at least thre_child
// times.  out[0] += |H|, out[1] += keys of H that A has, out[2] += the sum of A's clamped counts over H (both 0 without has_a).
__global__ __launch_bounds__(SP_THREADS) void hapmer_census_kernel(TableDev M, TableDev P, TableDev R, int has_r, TableDev A, int has_a, uint32_t thre, uint32_t thre_child,
                                                                   unsigned long long *__restrict__ out) {
    __shared__ unsigned long long s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t nslots = M.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    uint32_t nh = 0, nf = 0;
    unsigned long long occ = 0;
    for (uint64_t base = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; base < nslots; base += stride * SP_BATCH) {
        ulonglong2 e[SP_BATCH], ent[SP_BATCH];
        u128 h[SP_BATCH];
        bool cand[SP_BATCH];
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            e[u] = make_ulonglong2(0ull, 0ull);
            if (i < nslots) e[u] = *reinterpret_cast<const ulonglong2 *>(M.slots + 2 * i);   // tag + count, one 16-B load
        }
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            cand[u] = e[u].x != 0ull && e[u].y >= (unsigned long long)thre;      // (thre >= 1: a slot whose count is 0 is no key)
            h[u] = mk(0, 0);
            ent[u] = make_ulonglong2(0ull, 0ull);
            if (cand[u]) {
                h[u] = slot_hash(M, i, e[u].x);
                ent[u] = *reinterpret_cast<const ulonglong2 *>(P.slots + 2 * home_of(h[u], P.B, P.s));
            }
        }
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            if (!cand[u]) continue;
            if (table_get_prefetched(P, h[u], ent[u]) != 0ull) continue;
            if (has_r && clamp32(table_get(R, h[u])) < thre_child) continue;
            ++nh;
            if (has_a) {
                const uint32_t a = clamp32(table_get(A, h[u]));
                nf += a != 0u;
                occ += a;
            }
        }
    }
    nh = wave_sum(nh);
    nf = wave_sum(nf);
    occ = wave_sum(occ);
    if ((threadIdx.x & 63) == 0) {
        if (nh) atomicAdd(&s_sum[0], (unsigned long long)nh);
        if (nf) atomicAdd(&s_sum[1], (unsigned long long)nf);
        if (occ) atomicAdd(&s_sum[2], occ);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_sum[threadIdx.x]);
}

// what: "hap-mer scan", "hap-mer census" or "read bins" (readbins.hip).  R and A may be null.
int check_trio(const char *what, Table &M, Table &P, Table *R, Table *A, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child, std::string &err) {
    const std::string w(what);
    Table *all[4] = {&M, &P, R, A};
    const char *names[4] = {"maternal", "paternal", "child", "assembly"};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (all[i] && all[i] == all[j]) { err = w + ": the " + names[i] + " table and the " + names[j] + " table are the same table"; return -1; }
    for (int i = 1; i < 4; ++i) {
        if (!all[i]) continue;
        if (all[i]->k != M.k) {
            err = w + ": the tables have different k (" + names[0] + " " + std::to_string(M.k) + ", " + names[i] + " " + std::to_string(all[i]->k) + ")";
            return -1;
        }
        if (all[i]->device != M.device) { err = w + ": the tables are on different devices"; return -1; }
    }
    for (int i = 0; i < 4; ++i)
        if (i != 2 && all[i] && all[i]->d.nshard > 1) { err = w + ": the " + names[i] + " table must be a whole table, not an attached owner-sharded one"; return -1; }
    if (thre_mat < 1) { err = w + ": the maternal threshold must be at least 1 (it is 0)"; return -1; }
    if (thre_pat < 1) { err = w + ": the paternal threshold must be at least 1 (it is 0)"; return -1; }
    if (thre_child < 1) { err = w + ": the child threshold must be at least 1 (it is 0)"; return -1; }
    return 0;
}
namespace {
unsigned census_grid(uint64_t nslots) {                // as the spectrum's sweeps: fills the chip, the rest is grid-stride
    uint64_t b = (nslots + (uint64_t)SP_THREADS * SP_BATCH - 1) / ((uint64_t)SP_THREADS * SP_BATCH);
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), 256 * 8);
}
}  // namespace

int hapmer_scan_device(Table &M, Table &P, Table *R, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                       HapOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "hap-mer scan: bad arguments"; return -1; }
    if (check_trio("hap-mer scan", M, P, R, nullptr, thre_mat, thre_pat, thre_child, err)) return -1;
    Table &T = R ? *R : M;                              // whose stream and workspace the scan uses
    HIPCHK(hipSetDevice(T.device));
    Table *others[3] = {&M, &P, R};
    Events order;
    if (settle(T, others, 3, order, err)) return -1;
    return run_scan(T, Table::WS_HAPMERS, "hap-mer scan", n_seqs, d_text, offsets, HM_NCOUNT, 4, out.counts, out.runs, out.seconds, out.retried, err,
                    [&](unsigned grid, hipStream_t st, const TileList &L, uint64_t ntiles, unsigned long long *d_cnt, TileRuns *d_tout, HapRun *d_part, unsigned long long cap,
                        unsigned long long *d_ctl) {
                        hipLaunchKernelGGL(hapmer_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, M.d, P.d, R ? R->d : M.d, R ? 1 : 0, thre_mat,
                                           thre_pat, thre_child, d_cnt, d_tout, d_part, cap, d_ctl);
                    });
}

int hapmer_scan_host(Table &M, Table &P, Table *R, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                     HapOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "hap-mer scan: bad arguments"; return -1; }
    if (check_trio("hap-mer scan", M, P, R, nullptr, thre_mat, thre_pat, thre_child, err)) return -1;
    Table &T = R ? *R : M;
    HostText H;
    if (pack_host_text(T, Table::WS_HAPMERS, n_seqs, seqs, lens, "hap-mer scan", H, err)) return -1;
    return hapmer_scan_device(M, P, R, n_seqs, H.d_text, H.offs.data(), thre_mat, thre_pat, thre_child, out, err);
}

int hapmer_census(Table &M, Table &P, Table *R, Table *A, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child, uint64_t out6[6], double *seconds, std::string &err) {
    if (!out6) { err = "hap-mer census: null output"; return -1; }
    if (check_trio("hap-mer census", M, P, R, A, thre_mat, thre_pat, thre_child, err)) return -1;
    Table &T = R ? *R : M;
    HIPCHK(hipSetDevice(T.device));
    Table *others[4] = {&M, &P, R, A};
    Events order;
    if (settle(T, others, 4, order, err)) return -1;
    hipStream_t st = T.stream;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "census words");
    unsigned long long *d_out = (unsigned long long *)T.workspace(Table::WS_HAPMERS + 8, HC_WORDS * sizeof(unsigned long long), err);
    if (!d_out) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    HIPCHK(hipMemsetAsync(d_out, 0, HC_WORDS * sizeof(unsigned long long), st));
    HIPCHK(hipEventRecord(ev.e[0], st));
    const TableDev rd = R ? R->d : M.d, ad = A ? A->d : M.d;
    hipLaunchKernelGGL(hapmer_census_kernel, dim3(census_grid(M.nslots)), dim3(SP_THREADS), 0, st, M.d, P.d, rd, R ? 1 : 0, ad, A ? 1 : 0, thre_mat, thre_child, d_out);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hapmer_census_kernel, dim3(census_grid(P.nslots)), dim3(SP_THREADS), 0, st, P.d, M.d, rd, R ? 1 : 0, ad, A ? 1 : 0, thre_pat, thre_child, d_out + 3);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    unsigned long long res[HC_WORDS];
    HIPCHK(hipMemcpyAsync(res, d_out, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) *seconds = s;
    for (int i = 0; i < 6; ++i) out6[i] = res[i];
    return 0;
}

}  // namespace jk
