// diploid.hip -- both haplotypes of a diploid assembly against the reads: three resident tables of one k (reads R, assembly A1, other
// haplotype A2) joined on the device into P[4][10002], and the dense scan of ONE haplotype's sequences against R and the OTHER
// haplotype's table (semantics: include/jasper_hip.h, jasper_table_spectrum_pair and jasper_pair_scan).
//
// An extension the reference has no counterpart for (the diploid mode of a k-mer evaluation).  The join is spectra.hip's with one more
// table: a slot gives back its key's mixed hash, which does not depend on a table's size, so one hash probes both assembly tables.
//
//   spectra_pair_reads_kernel   sweep over the slots of R: slot -> hash -> count in A1 and in A2 -> bin [(in A1) | (in A2) << 1]
//                               [min(clamp32(count), 10001)].  sp_load has A1's home-slot loads in flight for the SP_BATCH slots of a
//                               thread; A2's go out right behind them, before any probe is resolved.  Columns below SP_LDS_COLS are
//                               binned in LDS (4 x 1024 x 4 B = 16 KB), the tail goes to the global matrix by 64-bit atomics; one flush
//                               per workgroup (sp_flush).
//   spectra_pair_asm_kernel     sweep over the slots of one assembly table S: slot -> hash -> count in R (loads of the batch in flight
//                               together) -> where R has none, a plain lookup in the other assembly table O under that branch (keys the
//                               reads do not hold are the assembly's errors: few).  Launched for A1 (alone -> row 1, with A2 -> row 3)
//                               and for A2 (alone -> row 2; the shared keys were A1's sweep's and are not counted again).  Two counters
//                               per thread, summed per wave, then per workgroup in LDS.
//   pair_scan_kernel            the dense scans' tile (scan_tile.hpp).  Per window ONE mix and TWO probes, R and O, both whole tables;
//                               the batching is the copy scan's (R's four home-slot loads in flight together, O's four go out as R's
//                               are resolved).  R's count stays in LDS (16 KB) with a 64-bit sum per group of 16; a thread's windows
//                               are two 16-bit class masks (private_solid / private_weak), which no window has both of.  Run starts, the
//                               walk through a class's masks and the tile's ends are the shared run finder; five adds per tile into the
//                               per-sequence counters.  It is not copies_scan_kernel with another classifier: it keeps no second count
//                               array and no second group sum (22 608 B of LDS where the copy scan has 41 048 B) and counts the report's two
//                               classes beside its own.
// The heads and stitch kernels and the host stage (settle, run_scan) are the shared ones of scan_tile.hpp; a solid run that a weak run
// follows directly gives two runs that touch, within a tile and across a seam (a run absorbs only partial runs of its kind).
#include "diploid.hpp"
#include "scan_tile.hpp"

namespace jk {

enum { PS_NCOUNT = 5 };                                                  // device counters per sequence: valid, unreliable, absent, private_solid, private_weak

__device__ __forceinline__ uint32_t kind_of(PairRun r) { return r.kind; }
__device__ __forceinline__ PairRun absorb(PairRun r, PairRun p) {
    r.n_kmers += p.n_kmers;
    r.sum_reads += p.sum_reads;
    return r;
}

__global__ __launch_bounds__(SP_THREADS) void spectra_pair_reads_kernel(TableDev R, TableDev A1, TableDev A2, unsigned long long *__restrict__ out) {
    __shared__ unsigned int bins[SPP_ROWS * SP_LDS_COLS];
    for (int i = threadIdx.x; i < SPP_ROWS * SP_LDS_COLS; i += SP_THREADS) bins[i] = 0;
    __syncthreads();
    const uint64_t nslots = R.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    for (uint64_t base = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; base < nslots; base += stride * SP_BATCH) {
        SpBatch b;
        ulonglong2 ent2[SP_BATCH];
        sp_load(R, R.slots, A1, base, stride, nslots, b);
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            ent2[u] = make_ulonglong2(0ull, 0ull);
            if (b.cnt[u] != 0ull) ent2[u] = *reinterpret_cast<const ulonglong2 *>(A2.slots + 2 * home_of(b.h[u], A2.B, A2.s));
        }
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            if (b.cnt[u] == 0ull) continue;
            const uint32_t in1 = table_get_prefetched(A1, b.h[u], b.ent[u]) != 0ull ? 1u : 0u;
            const uint32_t in2 = table_get_prefetched(A2, b.h[u], ent2[u]) != 0ull ? 2u : 0u;
            const uint32_t row = in1 | in2;
            const uint32_t c = clamp32(b.cnt[u]);
            const uint32_t col = c > (uint32_t)(SP_COLS - 1) ? (uint32_t)(SP_COLS - 1) : c;
            if (col < (uint32_t)SP_LDS_COLS) atomicAdd(&bins[row * SP_LDS_COLS + col], 1u);
            else atomicAdd(&out[(size_t)row * SP_COLS + col], 1ull);
        }
    }
    __syncthreads();
    sp_flush<SPP_ROWS>(bins, out);
}

// Sweep over the slots of S (one of the assembly tables): its keys that R does not hold go to column 0 of row_alone where O does not hold
// them either, and of row_both (0: not counted here) where it does.
__global__ __launch_bounds__(SP_THREADS) void spectra_pair_asm_kernel(TableDev S, TableDev R, TableDev O, uint32_t row_alone, uint32_t row_both,
                                                                      unsigned long long *__restrict__ out) {
    __shared__ unsigned int bins[2];
    if (threadIdx.x < 2) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t nslots = S.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    uint32_t na = 0, nb = 0;                             // keys of this thread that R does not hold: O neither / O does
    for (uint64_t base = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; base < nslots; base += stride * SP_BATCH) {
        SpBatch b;
        sp_load(S, S.slots, R, base, stride, nslots, b);
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            if (b.cnt[u] == 0ull) continue;
            if (table_get_prefetched(R, b.h[u], b.ent[u]) != 0ull) continue;
            const bool both = table_get(O, b.h[u]) != 0ull;      // (few keys come here: one dependent lookup, no registers held for it)
            na += both ? 0u : 1u;
            nb += both ? 1u : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        na += __shfl_xor(na, o);
        nb += __shfl_xor(nb, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (na) atomicAdd(&bins[0], na);
        if (nb) atomicAdd(&bins[1], nb);
    }
    __syncthreads();
    if (threadIdx.x == 0 && bins[0]) atomicAdd(&out[(size_t)row_alone * SP_COLS], (unsigned long long)bins[0]);
    if (threadIdx.x == 1 && bins[1] && row_both) atomicAdd(&out[(size_t)row_both * SP_COLS], (unsigned long long)bins[1]);
}

__global__ __launch_bounds__(RP_THREADS) void pair_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                               uint64_t ntiles, TableDev R, TableDev O, uint32_t thre, unsigned long long *__restrict__ counts,
                                                               TileRuns *__restrict__ tout, PairRun *__restrict__ part, unsigned long long cap,
                                                               unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_c[RP_TILE];                   // count in R of window w0 + i (0 where there is no k-mer)
    __shared__ uint32_t s_so[RP_THREADS];               // bit j of [g]: window w0 + 16g + j is `private_solid`
    __shared__ uint32_t s_we[RP_THREADS];               // ... is `private_weak`
    __shared__ unsigned long long s_gc[RP_THREADS];     // sum of s_c over group g
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot[PS_NCOUNT];               // valid, unreliable, absent, private_solid, private_weak windows of the tile
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const int k = R.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t < PS_NCOUNT) s_tot[t] = 0;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        uint32_t vm = 0, um = 0, am = 0, sm_ = 0, wm = 0;
        unsigned long long gc = 0;
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 er[4], eo[4];
            uint32_t cr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                ok[u] = roll_window(c, iv, j, k, kmask, R.B, e0, n, fwd, rc, run, hs[u]);
                er[u] = make_ulonglong2(0ull, 0ull);
                eo[u] = make_ulonglong2(0ull, 0ull);
                if (ok[u]) er[u] = *reinterpret_cast<const ulonglong2 *>(R.slots + 2 * home_of(hs[u], R.B, R.s));      // (R and O are whole tables)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                cr[u] = ok[u] ? clamp32(table_get_prefetched(R, hs[u], er[u])) : 0u;
                if (ok[u]) eo[u] = *reinterpret_cast<const ulonglong2 *>(O.slots + 2 * home_of(hs[u], O.B, O.s));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const bool priv = ok[u] && table_get_prefetched(O, hs[u], eo[u]) == 0ull;
                const bool un = ok[u] && cr[u] < thre;
                s_c[t * RP_GROUP + j] = cr[u];
                vm |= (ok[u] ? 1u : 0u) << j;
                um |= (un ? 1u : 0u) << j;
                am |= (ok[u] && cr[u] == 0u ? 1u : 0u) << j;
                sm_ |= (priv && !un ? 1u : 0u) << j;
                wm |= (priv && un ? 1u : 0u) << j;
                gc += cr[u];
            }
        }
        s_so[t] = sm_;
        s_we[t] = wm;
        s_gc[t] = gc;
        {
            const uint32_t cv = wave_sum(__popc(vm)), cu = wave_sum(__popc(um)), ca = wave_sum(__popc(am)), cs = wave_sum(__popc(sm_)), cw = wave_sum(__popc(wm));
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], cu);
                atomicAdd(&s_tot[2], ca);
                atomicAdd(&s_tot[3], cs);
                atomicAdd(&s_tot[4], cw);
            }
        }
        __syncthreads();
        // where my runs start: a class bit after a window that does not have that class (the tile's first window starts one anyway)
        const uint32_t ss = class_starts(sm_, s_so), sw = class_starts(wm, s_we);
        const uint32_t startmask = ss | sw;             // (no window has both classes)
        const uint32_t ns = __popc(startmask);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, tile_ends2(s_so, s_we, PS_SOLID, PS_WEAK)};
        if (t < PS_NCOUNT && s_tot[t]) atomicAdd(&counts[(unsigned long long)PS_NCOUNT * D.seq + t], (unsigned long long)s_tot[t]);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                const bool solid = (ss >> b0) & 1u;
                uint64_t sr = 0;
                PairRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = walk_run(solid ? s_so : s_we, t * RP_GROUP + b0, [&](int g, int, int pos, int len) {
                    if (len == RP_GROUP) sr += s_gc[g];           // whole groups by their stored sums
                    else
                        for (int j = 0; j < len; ++j) sr += s_c[pos + j];
                });
                r.sum_reads = sr;
                r.seq = D.seq;
                r.kind = solid ? PS_SOLID : PS_WEAK;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

namespace {
// what: "pair spectrum" or "pair scan".  names[i] is what tables[i] is called in the messages; tables[0] is the reads' table.
int check_tables(const char *what, Table *const *tables, const char *const *names, int n, std::string &err) {
    const std::string w(what);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (tables[i] == tables[j]) { err = w + ": the " + names[i] + " table and the " + names[j] + " table are the same table"; return -1; }
    for (int i = 1; i < n; ++i) {
        if (tables[i]->k != tables[0]->k) {
            err = w + ": the tables have different k (" + names[0] + " " + std::to_string(tables[0]->k) + ", " + names[i] + " " + std::to_string(tables[i]->k) + ")";
            return -1;
        }
        if (tables[i]->device != tables[0]->device) { err = w + ": the tables are on different devices"; return -1; }
    }
    for (int i = 0; i < n; ++i)
        if (tables[i]->d.nshard > 1) { err = w + ": the " + names[i] + " table must be a whole table, not an attached owner-sharded one"; return -1; }
    return 0;
}
}  // namespace

int table_spectrum_pair(Table &R, Table &A1, Table &A2, uint64_t *out, double *seconds, std::string &err) {
    if (!out) { err = "pair spectrum: null output"; return -1; }
    Table *tables[3] = {&R, &A1, &A2};
    const char *names[3] = {"read", "assembly", "alt"};
    if (check_tables("pair spectrum", tables, names, 3, err)) return -1;
    HIPCHK(hipSetDevice(R.device));
    Table *others[2] = {&A1, &A2};                      // a logically empty table holds garbage until it is zeroed: all three are swept and probed
    Events order;
    if (settle(R, others, 2, order, err)) return -1;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "spectrum words");
    const size_t bytes = (size_t)SPP_ROWS * SP_COLS * sizeof(unsigned long long);
    unsigned long long *d_out = (unsigned long long *)R.workspace(Table::WS_DIPLOID, bytes, err);
    if (!d_out) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    hipStream_t st = R.stream;
    HIPCHK(hipMemsetAsync(d_out, 0, bytes, st));
    HIPCHK(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(spectra_pair_reads_kernel, dim3(sweep_grid(R.nslots)), dim3(SP_THREADS), 0, st, R.d, A1.d, A2.d, d_out);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(spectra_pair_asm_kernel, dim3(sweep_grid(A1.nslots)), dim3(SP_THREADS), 0, st, A1.d, R.d, A2.d, 1u, 3u, d_out);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(spectra_pair_asm_kernel, dim3(sweep_grid(A2.nslots)), dim3(SP_THREADS), 0, st, A2.d, R.d, A1.d, 2u, 0u, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    HIPCHK(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) *seconds = s;
    return 0;
}

int pair_scan_host(Table &R, Table &O, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, PairOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "pair scan: bad arguments"; return -1; }
    Table *tables[2] = {&R, &O};
    const char *names[2] = {"read", "other haplotype's"};
    if (check_tables("pair scan", tables, names, 2, err)) return -1;
    const int W = Table::WS_DIPLOID + 1;                // (slot WS_DIPLOID is the pair spectrum's matrix)
    HostText H;
    if (pack_host_text(R, W, n_seqs, seqs, lens, "pair scan", H, err)) return -1;
    HIPCHK(hipSetDevice(R.device));
    Table *others[1] = {&O};                            // a logically empty table holds garbage until it is zeroed: both tables are probed
    Events order;
    if (settle(R, others, 1, order, err)) return -1;
    const uint8_t *d_text = H.d_text;
    return run_scan(R, W, "pair scan", n_seqs, d_text, H.offs.data(), PS_NCOUNT, 6, out.counts, out.runs, out.seconds, out.retried, err,
                    [&](unsigned grid, hipStream_t st, const TileList &L, uint64_t ntiles, unsigned long long *d_cnt, TileRuns *d_tout, PairRun *d_part, unsigned long long cap,
                        unsigned long long *d_ctl) {
                        hipLaunchKernelGGL(pair_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, R.d, O.d, thre, d_cnt, d_tout, d_part, cap,
                                           d_ctl);
                    });
}

}  // namespace jk
