// copies.hip -- copy-number scan: every window of every sequence looked up in the reads' table R and in the assembly's table A,
// classified by the copy number the reads support against the copies the assembly holds, as per-sequence counters and the maximal
// runs of each class (semantics: include/jasper_hip.h, jasper_copy_report).
//
// An extension the reference has no counterpart for.  It is the dense scan of report.hip joined with the second table of
// spectra.hip: the spectrum says how many distinct k-mers are collapsed or duplicated, this says where on the contigs they are.
//
//   copies_scan_kernel    the dense scans' tile (scan_tile.hpp: staging with the 64-base halo, the rolling state before a thread's
//                         first window, the reservation of places in the list).  Per window ONE mix (the hash does not depend on a
//                         table's size) and TWO probes: R through read_slots (the owner's shard when R is attached), A whole.  The
//                         home-slot loads of a batch of four windows
//                         are in flight before any is resolved; A's four loads go out after R's four are resolved (CP_A_EARLY: with
//                         them -- DESIGN 4.5 has both measurements).  Both counts stay in LDS (2 x 16 KB) with a 64-bit sum per
//                         group of 16; a thread's windows are two 16-bit class masks (excess / deficit).  A run starts where a class
//                         bit follows a window that does not have that class (clear, the other class, the thread before's last
//                         window) or at the tile's first window, and every start walks its run through its class's masks -- whole
//                         groups by their stored sums -- to the run's or the tile's end (class_starts, tile_ends2 and walk_run of
//                         scan_tile.hpp; the sums per piece of a run are this kernel's).  The tile's PARTIAL runs go to a list (one
//                         cursor add per tile) with the class of the tile's first and last window; five adds per tile into the
//                         per-sequence counters.  Nothing per window leaves the CU.
// A window's rolling step, the run finder, the heads and stitch kernels that make final runs of the partial ones, and the host stage
// (run_scan; settle orders A's stream before R's) are the shared ones of scan_tile.hpp; a run continues across a tile seam when both
// sides have the same non-zero class, and absorbs only partial runs OF ITS KIND.
//
// The class of a window needs e = (2c + peak) div (2 peak) only in comparison with a; with P = peak * a (< 2^64):
//   e > a  <=>  (2c + peak) / (2 peak) >= a + 1  <=>  2c >= 2P + peak        e < a  <=>  (2c + peak) / (2 peak) < a  <=>  2c + peak < 2P
// and 2c + peak < 2^34, so P >= 2^33 decides both without forming 2P: no 64-bit division per window, the same classes.
//
// The list of partial runs starts at windows / 64 + 64K entries, as the report's; a scan that needed more has counted how many and
// is repeated once with exactly that room.
#include "copies.hpp"
#include "scan_tile.hpp"

#ifndef CP_A_EARLY
#define CP_A_EARLY 0
#endif
#ifndef CP_BATCH_UNROLL
#define CP_BATCH_UNROLL 1      // 1: the four batches of a thread as a loop, 4: unrolled (registers against occupancy)
#endif
#define CP_STR_(x) #x
#define CP_PRAGMA_UNROLL(n) _Pragma(CP_STR_(unroll n))

namespace jk {

enum { CP_NCOUNT = 5 };                                                  // device counters per sequence: valid, excess, deficit, sum_reads, sum_asm

__device__ __forceinline__ uint32_t kind_of(CopyRun r) { return r.kind; }
__device__ __forceinline__ CopyRun absorb(CopyRun r, CopyRun p) {
    r.n_kmers += p.n_kmers;
    r.sum_reads += p.sum_reads;
    r.sum_asm += p.sum_asm;
    return r;
}

__global__ __launch_bounds__(RP_THREADS) void copies_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                                 uint64_t ntiles, TableDev R, TableDev A, uint32_t thre, uint32_t peak,
                                                                 unsigned long long *__restrict__ counts, TileRuns *__restrict__ tout, CopyRun *__restrict__ part,
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
    const int t = threadIdx.x, lane = t & 63;
    const int k = R.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t < 3) s_tot[t] = 0;
        if (t < 2) s_sum[t] = 0ull;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
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
                ok[u] = roll_window(c, iv, j, k, kmask, R.B, e0, n, fwd, rc, run, hs[u]);
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
            const uint32_t cv = wave_sum(__popc(vm)), ce = wave_sum(__popc(em)), cd = wave_sum(__popc(dm));
            const unsigned long long sc = wave_sum(gc), sa = wave_sum(ga);
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
        const uint32_t se = class_starts(em, s_ex), sd = class_starts(dm, s_de);
        const uint32_t startmask = se | sd;             // (no window has both classes)
        const uint32_t ns = __popc(startmask);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, tile_ends2(s_ex, s_de, CP_EXCESS, CP_DEFICIT)};
        if (t < 3 && s_tot[t]) atomicAdd(&counts[(unsigned long long)CP_NCOUNT * D.seq + t], (unsigned long long)s_tot[t]);
        if (t >= 3 && t < 5 && s_sum[t - 3]) atomicAdd(&counts[(unsigned long long)CP_NCOUNT * D.seq + t], s_sum[t - 3]);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                const bool isex = (se >> b0) & 1u;
                uint64_t sr = 0, sa = 0;
                CopyRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = walk_run(isex ? s_ex : s_de, t * RP_GROUP + b0, [&](int g, int, int pos, int len) {
                    if (len == RP_GROUP) {                        // whole groups by their stored sums
                        sr += s_gc[g];
                        sa += s_ga[g];
                    } else {
                        for (int j = 0; j < len; ++j) {
                            sr += s_c[pos + j];
                            sa += s_a[pos + j];
                        }
                    }
                });
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

namespace {
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
    Table *others[1] = {&A};                            // a logically empty table holds garbage until it is zeroed: both tables are probed
    Events order;
    if (settle(R, others, 1, order, err)) return -1;
    return run_scan(R, Table::WS_COPIES, "copy report", n_seqs, d_text, offsets, CP_NCOUNT, 6, out.counts, out.runs, out.seconds, out.retried, err,
                    [&](unsigned grid, hipStream_t st, const TileList &L, uint64_t ntiles, unsigned long long *d_cnt, TileRuns *d_tout, CopyRun *d_part, unsigned long long cap,
                        unsigned long long *d_ctl) {
                        hipLaunchKernelGGL(copies_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, R.d, A.d, thre, peak, d_cnt, d_tout, d_part,
                                           cap, d_ctl);
                    });
}

int copies_report_host(Table &R, Table &A, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak, CopyOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "copy report: bad arguments"; return -1; }
    if (check_pair(R, A, peak, err)) return -1;
    HostText H;
    if (pack_host_text(R, Table::WS_COPIES, n_seqs, seqs, lens, "copy report", H, err)) return -1;
    return copies_report_device(R, A, n_seqs, H.d_text, H.offs.data(), thre, peak, out, err);
}

}  // namespace jk
