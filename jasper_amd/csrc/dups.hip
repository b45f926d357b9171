// dups.hip -- duplication map: every window whose k-mer the assembly's table A holds exactly twice paired with the place of the other
// copy, and the maximal colinear runs of such pairs with what the reads' table R says about them (semantics: include/jasper_hip.h,
// jasper_dup_map).
//
// An extension the reference has no counterpart for.  The copy scan (copies.hip) finds `deficit` runs -- the assembly holds a stretch
// more often than the reads support -- and cannot say where the other copy is: the tables hold counts, not places.  Two dense scans of
// the text get the places:
//
//   dup_index_kernel      the dense scans' tile (scan_tile.hpp) with ONE probe of A per window, a batch of four home-slot loads in
//                         flight before any is resolved.  For a window whose k-mer has count 2 the encoded position (global position
//                         and strand bit, dup_encode) goes into the slot's two side words with a 64-bit atomicMin and atomicMax:
//                         whatever the order, the words end as the smaller and the larger of the k-mer's two places.  table_find is
//                         table_get's probe loop returning the slot as well as the count.
//   dup_scan_kernel       the same tile.  Per window the probe of R, the probe of A and, for count 2, one 16-byte load of the side
//                         words.  A window is two-copy when the words are two places and one is its own; the other is its mate.  Its
//                         pairing key is the orientation (the two strand bits differ or not) and the diagonal (mate - position for
//                         `+`, mate + position for `-`): two neighbours belong to one run exactly when both are two-copy and have one
//                         key.  A thread keeps its sixteen keys in registers and compares them there; only its last key goes to LDS,
//                         for the thread after it, and thread 0 looks up the window before the tile (one more window's lookups per
//                         tile; the tile's prologue has its k-mer already).  The `cont` bit of a window says it continues the window
//                         before; runs start at two_copy & ~cont and at the tile's first window, and walk_run over the cont masks
//                         gives their lengths, read sums (whole groups by their stored sums) and deficit windows.
// The tile's ends for the shared stitcher: first class 1 exactly when the first window continues the window before the tile, last class
// 1 when the last window is two-copy.  A run that continues across a seam absorbs the next tile's first partial run and keeps its own
// mate; the stitch kernels and the host stage are the shared ones, unchanged.
//
// A partial run carries the global position of its first window's mate; dups_host.hpp makes (sequence, leftmost window) of it.
#include "dups.hpp"
#include "scan_tile.hpp"

namespace jk {

enum { DP_NCOUNT = 6 };                                                  // device counters per sequence: valid, two_copy, deficit, multi, unplaced, sum_reads
constexpr uint64_t DP_NONE = ~0ull;

__device__ __forceinline__ uint32_t kind_of(DupRun) { return 1u; }       // one class: the tile's ends say what continues
__device__ __forceinline__ DupRun absorb(DupRun r, DupRun p) {
    r.n_kmers += p.n_kmers;
    r.sum_reads += p.sum_reads;
    r.n_deficit += p.n_deficit;
    return r;                                                            // (the head's mate stays)
}

// The slot of the key whose mixed hash is h, or DP_NONE, and its 64-bit count (0 without a slot): table_get's probe loop, narrow and
// wide tables alike.
__device__ __forceinline__ uint64_t table_find(const TableDev &T, u128 h, unsigned long long &count) {
    const uint64_t home = home_of(h, T.B, T.s);
    const uint64_t rem = tag_rem_of(h, T.B, T.s);
    const unsigned long long *S = read_slots(T, h);
    const bool wide = T.ext != nullptr;
    const unsigned long long ext = wide ? ext_of(h, T.B, T.s) : 0ull;
    count = 0ull;
    for (uint32_t off = 0; off < MAXPROBE; ++off) {
        const uint64_t slot = (home + off) & T.mask;
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(S + 2 * slot);
        if (e.x == tag_of(rem, off) && (!wide || T.ext[slot] == ext)) {
            count = e.y;
            return slot;
        }
        if (e.x == 0ull) return DP_NONE;
    }
    return DP_NONE;
}
// the same with the home slot already loaded
__device__ __forceinline__ uint64_t table_find_prefetched(const TableDev &T, u128 h, ulonglong2 e0, unsigned long long &count) {
    if (T.ext) return table_find(T, h, count);
    const uint64_t home = home_of(h, T.B, T.s);
    const uint64_t rem = rem_of(h, T.B, T.s);
    count = 0ull;
    if (e0.x == tag_of(rem, 0)) {
        count = e0.y;
        return home & T.mask;
    }
    if (e0.x == 0ull) return DP_NONE;
    const unsigned long long *S = read_slots(T, h);
    for (uint32_t off = 1; off < MAXPROBE; ++off) {
        const uint64_t slot = (home + off) & T.mask;
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(S + 2 * slot);
        if (e.x == tag_of(rem, off)) {
            count = e.y;
            return slot;
        }
        if (e.x == 0ull) return DP_NONE;
    }
    return DP_NONE;
}

// every slot's side words as "no place seen": the smallest above every position, the largest below
__global__ __launch_bounds__(256) void dup_fill_kernel(ulonglong2 *__restrict__ side, uint64_t nslots) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) side[i] = make_ulonglong2(~0ull, 0ull);
}

__global__ __launch_bounds__(RP_THREADS) void dup_index_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                               uint64_t ntiles, TableDev A, unsigned long long *__restrict__ side) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    const int t = threadIdx.x;
    const int k = A.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        const int64_t g0 = offs[D.seq] + w0 + (int64_t)t * RP_GROUP;      // global position of my first window
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            uint32_t sb[4];
            ulonglong2 ea[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ok[u] = roll_window(c, iv, j0 + u, k, kmask, A.B, e0, n, fwd, rc, run, hs[u]);
                sb[u] = lt(rc, fwd) ? 1u : 0u;
                ea[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) ea[u] = *reinterpret_cast<const ulonglong2 *>(A.slots + 2 * home_of(hs[u], A.B, A.s));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                unsigned long long a;
                const uint64_t slot = table_find_prefetched(A, hs[u], ea[u], a);
                if (slot != DP_NONE && a == 2ull) {
                    const unsigned long long enc = ((unsigned long long)(g0 + j0 + u) << 1) | sb[u];
                    atomicMin(&side[2 * slot], enc);
                    atomicMax(&side[2 * slot + 1], enc);
                }
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

// A window at global position gpos with strand bit sb whose k-mer has count 2 and the side words m: is it two-copy, and its pairing key
__device__ __forceinline__ bool dup_pair(ulonglong2 m, int64_t gpos, uint32_t sb, uint32_t &minus, int64_t &diag) {
    const unsigned long long own = ((unsigned long long)gpos << 1) | sb;
    const bool two = m.x != m.y && (own == m.x || own == m.y);
    const unsigned long long mate = own == m.x ? m.y : m.x;
    const int64_t mpos = (int64_t)(mate >> 1);
    minus = (uint32_t)((mate ^ own) & 1ull);
    diag = minus ? mpos + gpos : mpos - gpos;
    return two;
}

__global__ __launch_bounds__(RP_THREADS) void dup_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                              uint64_t ntiles, TableDev R, TableDev A, const unsigned long long *__restrict__ side, uint32_t thre,
                                                              uint32_t peak, unsigned long long *__restrict__ counts, TileRuns *__restrict__ tout,
                                                              DupRun *__restrict__ part, unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_c[RP_TILE];                   // count in R of window w0 + i (0 where there is no k-mer)
    __shared__ uint32_t s_cont[RP_THREADS];             // bit j of [g]: window w0 + 16g + j continues the window before it
    __shared__ uint32_t s_de[RP_THREADS];               // ... is two-copy and `deficit`
    __shared__ unsigned long long s_gc[RP_THREADS];     // sum of s_c over the two-copy windows of group g
    __shared__ long long s_key[RP_THREADS];             // the diagonal of thread g's last window ...
    __shared__ uint32_t s_kf[RP_THREADS];               // ... bit 0: it is two-copy, bit 1: its orientation is `-`
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot[5];                       // valid, two-copy, deficit, multi, unplaced windows of the tile
    __shared__ unsigned long long s_sum;                // sum of c over the tile's two-copy windows
    __shared__ uint32_t s_last;                         // the tile's last window is two-copy
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const int k = R.k;
    const u128 kmask = maskbits(2 * k);
    const unsigned long long peak3 = 3ull * peak;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t < 5) s_tot[t] = 0;
        if (t == 5) s_sum = 0ull;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        const int64_t g0 = offs[D.seq] + w0 + (int64_t)t * RP_GROUP;      // global position of my first window
        // the window before the tile, for thread 0 alone: the prologue's k-mer is its k-mer
        uint32_t pflag = 0;
        int64_t pdiag = 0;
        if (t == 0 && D.idx > 0 && run >= k) {
            const bool rcan = lt(rc, fwd);
            unsigned long long a;
            const uint64_t slot = table_find(A, mix(rcan ? rc : fwd, A.B), a);
            if (slot != DP_NONE && a == 2ull) {
                uint32_t minus;
                const bool two = dup_pair(*reinterpret_cast<const ulonglong2 *>(side + 2 * slot), g0 - 1, rcan ? 1u : 0u, minus, pdiag);
                pflag = (two ? 1u : 0u) | (minus << 1);
            }
        }
        uint32_t vm = 0, tm = 0, om = 0, dm = 0, mm = 0, um = 0;
        unsigned long long gc = 0;
        int64_t diag[RP_GROUP];
#pragma unroll
        for (int j = 0; j < RP_GROUP; ++j) diag[j] = 0;
#pragma unroll 1
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {      // (rolled: four unrolled batches cost a third of the occupancy)
            u128 hs[4];
            bool ok[4];
            uint32_t sb[4], cr[4];
            ulonglong2 er[4], ea[4], ms[4];
            unsigned long long aa[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ok[u] = roll_window(c, iv, j0 + u, k, kmask, R.B, e0, n, fwd, rc, run, hs[u]);
                sb[u] = lt(rc, fwd) ? 1u : 0u;
                er[u] = make_ulonglong2(0ull, 0ull);
                ea[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) er[u] = *reinterpret_cast<const ulonglong2 *>(read_slots(R, hs[u]) + 2 * home_of(hs[u], R.B, R.s));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                cr[u] = ok[u] ? clamp32(table_get_prefetched(R, hs[u], er[u])) : 0u;
                if (ok[u]) ea[u] = *reinterpret_cast<const ulonglong2 *>(A.slots + 2 * home_of(hs[u], A.B, A.s));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                aa[u] = 0ull;
                ms[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) {
                    const uint64_t slot = table_find_prefetched(A, hs[u], ea[u], aa[u]);
                    if (slot != DP_NONE && aa[u] == 2ull) ms[u] = *reinterpret_cast<const ulonglong2 *>(side + 2 * slot);      // (16 bytes, in flight for all four)
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                uint32_t minus = 0;
                int64_t dg = 0;
                const bool two = ok[u] && aa[u] == 2ull && dup_pair(ms[u], g0 + j, sb[u], minus, dg);
                const bool de = two && cr[u] >= thre && 2ull * cr[u] < peak3;      // (2c + peak) div (2 peak) < 2
#pragma unroll
                for (int q = 0; q < RP_GROUP / 4; ++q) diag[4 * q + u] = j0 == 4 * q ? dg : diag[4 * q + u];      // (selects on constant indices: no scratch)
                s_c[t * RP_GROUP + j] = cr[u];
                vm |= (ok[u] ? 1u : 0u) << j;
                tm |= (two ? 1u : 0u) << j;
                om |= (two ? minus : 0u) << j;
                dm |= (de ? 1u : 0u) << j;
                mm |= (ok[u] && aa[u] >= 3ull ? 1u : 0u) << j;
                um |= (ok[u] && aa[u] == 2ull && !two ? 1u : 0u) << j;
                gc += two ? cr[u] : 0u;
            }
        }
        s_de[t] = dm;
        s_gc[t] = gc;
        s_key[t] = diag[RP_GROUP - 1];
        s_kf[t] = ((tm >> 15) & 1u) | (((om >> 15) & 1u) << 1);
        if (t == RP_THREADS - 1) s_last = (tm >> 15) & 1u;
        {
            const uint32_t cv = wave_sum(__popc(vm)), ct = wave_sum(__popc(tm)), cd = wave_sum(__popc(dm)), cm = wave_sum(__popc(mm)), cu = wave_sum(__popc(um));
            const unsigned long long sc = wave_sum(gc);
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], ct);
                atomicAdd(&s_tot[2], cd);
                atomicAdd(&s_tot[3], cm);
                atomicAdd(&s_tot[4], cu);
                atomicAdd(&s_sum, sc);
            }
        }
        __syncthreads();
        // which of my windows continue the one before: both two-copy, one orientation, one diagonal
        if (t > 0) {
            pflag = s_kf[t - 1];
            pdiag = s_key[t - 1];
        }
        uint32_t cont = (tm & 1u) && (pflag & 1u) && ((pflag >> 1) & 1u) == (om & 1u) && pdiag == diag[0] ? 1u : 0u;
#pragma unroll
        for (int j = 1; j < RP_GROUP; ++j)
            cont |= (((tm >> j) & (tm >> (j - 1)) & 1u) && ((om >> j) & 1u) == ((om >> (j - 1)) & 1u) && diag[j] == diag[j - 1] ? 1u : 0u) << j;
        s_cont[t] = cont;
        const uint32_t startmask = (tm & ~cont) | (t == 0 ? tm & 1u : 0u);      // (the tile's first window starts a partial run anyway)
        const uint32_t ns = __popc(startmask);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);   // (its barrier: s_cont is whole)
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, (cont & 1u) | (s_last << 2)};
        if (t < 5 && s_tot[t]) atomicAdd(&counts[(unsigned long long)DP_NCOUNT * D.seq + t], (unsigned long long)s_tot[t]);
        if (t == 5 && s_sum) atomicAdd(&counts[(unsigned long long)DP_NCOUNT * D.seq + 5], s_sum);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                int64_t dg = 0;
#pragma unroll
                for (int j = 0; j < RP_GROUP; ++j) dg = j == b0 ? diag[j] : dg;      // (selects on constant indices: no scratch)
                const uint32_t minus = (om >> b0) & 1u;
                const int pos = t * RP_GROUP + b0;
                const int64_t gpos = g0 + b0;
                uint64_t sr = s_c[pos], nd = (dm >> b0) & 1u;
                DupRun r;
                r.start = w0 + pos;
                r.mate_start = minus ? dg - gpos : dg + gpos;      // the mate of the run's first window, a global position
                r.n_kmers = 1 + walk_run(s_cont, pos + 1, [&](int g, int b, int p, int len) {
                    if (len == RP_GROUP) {                        // whole groups by their stored sums
                        sr += s_gc[g];
                        nd += __popc(s_de[g]);
                    } else {
                        for (int j = 0; j < len; ++j) sr += s_c[p + j];
                        nd += __popc((s_de[g] >> b) & ((1u << len) - 1u));
                    }
                });
                r.sum_reads = sr;
                r.n_deficit = nd;
                r.seq = D.seq;
                r.mate_seq = 0;
                r.strand = minus;
                r.pad = 0;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

namespace {
int check_pair(Table &R, Table &A, uint32_t peak, std::string &err) {
    if (&R == &A) { err = "duplication map: the read table and the assembly table are the same table"; return -1; }
    if (R.k != A.k) { err = "duplication map: the tables have different k (" + std::to_string(R.k) + " and " + std::to_string(A.k) + ")"; return -1; }
    if (R.device != A.device) { err = "duplication map: the tables are on different devices"; return -1; }
    if (A.d.nshard > 1) { err = "duplication map: the assembly table must be a whole table, not an attached owner-sharded one"; return -1; }
    if (peak < 1) { err = "duplication map: peak must be at least 1"; return -1; }
    return 0;
}
}  // namespace

int dup_map_device(Table &R, Table &A, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak, DupOut &out, std::string &err) {
    const char *what = "duplication map";
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "duplication map: bad arguments"; return -1; }
    if (check_pair(R, A, peak, err)) return -1;
    HIPCHK(hipSetDevice(R.device));
    Table *others[1] = {&A};                            // a logically empty table holds garbage until it is zeroed: both tables are probed
    Events order;
    if (settle(R, others, 1, order, err)) return -1;
    out.index_seconds = 0;
    // pass 1: the places of A's count-2 k-mers into the side array (the tiles are the scan's own; run_scan uploads the same list again)
    TileList L;
    if (build_tiles(R.k, n_seqs, d_text, offsets, what, nullptr, 0, L, err)) return -1;
    const uint64_t ntiles = L.tiles.size(), nslots = A.d.mask + 1;
    unsigned long long *d_side = nullptr;
    Events ev;
    if (ntiles) {
        hipStream_t st = R.stream;
        d_side = (unsigned long long *)R.workspace(Table::WS_DUPS + 8, nslots * 2 * sizeof(unsigned long long), err);
        if (!d_side || upload_tiles(R, Table::WS_DUPS, n_seqs, offsets, L, err) || ev.create(err)) return -1;
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(dup_fill_kernel, dim3((unsigned)std::min<uint64_t>((nslots + 255) / 256, 256 * 32)), dim3(256), 0, st, (ulonglong2 *)d_side, nslots);
        hipLaunchKernelGGL(dup_index_kernel, dim3((unsigned)std::min<uint64_t>(ntiles, 256 * 8)), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, A.d, d_side);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
    }
    // pass 2: the join and the runs
    if (run_scan(R, Table::WS_DUPS, what, n_seqs, d_text, offsets, DP_NCOUNT, 7, out.counts, out.runs, out.seconds, out.retried, err,
                 [&](unsigned grid, hipStream_t st, const TileList &T, uint64_t nt, unsigned long long *d_cnt, TileRuns *d_tout, DupRun *d_part, unsigned long long cap,
                     unsigned long long *d_ctl) {
                     hipLaunchKernelGGL(dup_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, T.d_offs, T.d_tiles, nt, R.d, A.d, d_side, thre, peak, d_cnt, d_tout,
                                        d_part, cap, d_ctl);
                 }))
        return -1;
    if (ntiles && ev.add_seconds(out.index_seconds, err)) return -1;      // (run_scan has waited for the stream)
    return dup_finish_runs(out.runs, R.k, n_seqs, offsets, err);
}

int dup_map_host(Table &R, Table &A, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak, DupOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "duplication map: bad arguments"; return -1; }
    if (check_pair(R, A, peak, err)) return -1;
    HostText H;
    if (pack_host_text(R, Table::WS_DUPS, n_seqs, seqs, lens, "duplication map", H, err)) return -1;
    return dup_map_device(R, A, n_seqs, H.d_text, H.offs.data(), thre, peak, out, err);
}

}  // namespace jk
