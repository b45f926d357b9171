// report.hip -- dense k-mer report: per-sequence counters and the maximal runs of unreliable windows, from the resident table.
//
// An extension the reference has no counterpart for.  The windows are those of src/jasper.py:55-71 (a window is looked up iff all
// its k bytes are ACGTacgt), but EVERY window of every sequence is taken, not the strided walk of the QV pass, and sequences are
// whole (nothing is cut at chunk records).  The counts are what jasper_lookup reports: the canonical k-mer's, clamped to 2^32-1.
//
//   report_scan_kernel    a tile of RP_TILE windows of ONE sequence per workgroup iteration.  Staging, rolling and the four home-slot
//                         loads in flight are those of the polisher's dense scan (thread t owns the 16 windows that end at
//                         origin + 16t ..); what follows the count is new: counts and class bits stay in LDS, a thread's 16 windows
//                         are three 16-bit masks (valid / unreliable / absent), a run starts where an unreliable bit follows a
//                         clear one (or at the tile's first window), and every start walks its run through the masks -- whole
//                         groups by their stored minimum -- to the run's or the tile's end.  The tile's PARTIAL runs go to a list
//                         (one cursor add per tile), with "open at the tile's start / end" marks; the per-sequence counters get
//                         three adds per tile.  Nothing per window leaves the CU.
//
// The tile's front end (staging, the rolling state before a thread's first window), a window's rolling step, the reservation of places in
// the list, the run finder (run starts, the tile's ends, the walk through a class's masks), the heads and stitch kernels that make final
// runs of the partial ones, and the host stage (text packing, tile list, the repeat with exactly the counted room) are the dense scans'
// common parts: scan_tile.hpp.  Here the report has one class, unreliable = 1, and its own accumulation per piece of a run.
#include "scan_tile.hpp"

namespace jk {

__device__ __forceinline__ uint32_t kind_of(KmerRun) { return 1u; }
__device__ __forceinline__ KmerRun absorb(KmerRun r, KmerRun p) {
    r.n_kmers += p.n_kmers;
    r.n_absent += p.n_absent;
    r.min_count = min(r.min_count, p.min_count);
    return r;
}

__global__ __launch_bounds__(RP_THREADS) void report_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                                 uint64_t ntiles, TableDev T, uint32_t thre, unsigned long long *__restrict__ counts,
                                                                 TileRuns *__restrict__ tout, KmerRun *__restrict__ part, unsigned long long cap,
                                                                 unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_cnt[RP_TILE];                 // count of window w0 + i (0 where there is no k-mer)
    __shared__ uint32_t s_unrel[RP_THREADS];            // bit j of [g]: window w0 + 16g + j is unreliable
    __shared__ uint32_t s_abs[RP_THREADS];              // ... is absent
    __shared__ uint32_t s_gmin[RP_THREADS];             // smallest count among the unreliable windows of group g
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot[3];                       // valid, unreliable, absent windows of the tile
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const int k = T.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t < 3) s_tot[t] = 0;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        uint32_t vm = 0, um = 0, am = 0, gmin = 0xFFFFFFFFu;
#pragma unroll
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 ent[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                ok[u] = roll_window(c, iv, j, k, kmask, T.B, e0, n, fwd, rc, run, hs[u]);
                ent[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) ent[u] = *reinterpret_cast<const ulonglong2 *>(read_slots(T, hs[u]) + 2 * home_of(hs[u], T.B, T.s));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const uint32_t cnt = ok[u] ? clamp32(table_get_prefetched(T, hs[u], ent[u])) : 0u;
                const bool un = ok[u] && cnt < thre;
                s_cnt[t * RP_GROUP + j] = cnt;
                vm |= (ok[u] ? 1u : 0u) << j;
                um |= (un ? 1u : 0u) << j;
                am |= (ok[u] && cnt == 0u ? 1u : 0u) << j;
                gmin = un && cnt < gmin ? cnt : gmin;
            }
        }
        s_unrel[t] = um;
        s_abs[t] = am;
        s_gmin[t] = gmin;
        {
            const uint32_t cv = wave_sum(__popc(vm)), cu = wave_sum(__popc(um)), ca = wave_sum(__popc(am));
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], cu);
                atomicAdd(&s_tot[2], ca);
            }
        }
        __syncthreads();
        // where my runs start: an unreliable window after one that is not (the tile's first window starts one anyway)
        const uint32_t startmask = class_starts(um, s_unrel);
        const uint32_t ns = __popc(startmask);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, tile_ends(s_unrel)};
        if (t < 3 && s_tot[t]) atomicAdd(&counts[3ull * D.seq + t], (unsigned long long)s_tot[t]);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                uint64_t na = 0;
                uint32_t mn = 0xFFFFFFFFu;
                KmerRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = walk_run(s_unrel, t * RP_GROUP + b0, [&](int g, int b, int pos, int len) {
                    if (len == RP_GROUP) mn = min(mn, s_gmin[g]);      // whole groups by their stored minimum
                    else
                        for (int j = 0; j < len; ++j) mn = min(mn, s_cnt[pos + j]);
                    na += __popc((s_abs[g] >> b) & ((1u << len) - 1u));
                });
                r.n_absent = na;
                r.seq = D.seq;
                r.min_count = mn;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

int kmer_report_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, ReportOut &R, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "kmer report: bad arguments"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    if (T.materialize(err)) return -1;
    return run_scan(T, Table::WS_REPORT, "kmer report", n_seqs, d_text, offsets, 3, 4, R.counts, R.runs, R.seconds, R.retried, err,
                    [&](unsigned grid, hipStream_t st, const TileList &L, uint64_t ntiles, unsigned long long *d_cnt, TileRuns *d_tout, KmerRun *d_part, unsigned long long cap,
                        unsigned long long *d_ctl) {
                        hipLaunchKernelGGL(report_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, T.d, thre, d_cnt, d_tout, d_part, cap, d_ctl);
                    });
}

int kmer_report_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, ReportOut &R, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "kmer report: bad arguments"; return -1; }
    HostText H;
    if (pack_host_text(T, Table::WS_REPORT, n_seqs, seqs, lens, "kmer report", H, err)) return -1;
    return kmer_report_device(T, n_seqs, H.d_text, H.offs.data(), thre, R, err);
}

}  // namespace jk
