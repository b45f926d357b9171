// gaps.hip -- gap scan: what the reads hold in place of a scaffold gap or of a long run of unreliable k-mers (semantics:
// include/jasper_hip.h, jasper_gap_scan).
//
// An extension.  The dense scan is the report's (report.hip), unchanged: its runs are the unreliable windows.  The windows that hold a
// non-base byte -- which no scan here lists, because they have no k-mer -- come from
//
//   gap_runs_kernel      a run scan with ONE class, "this window has no k-mer", on the common parts of scan_tile.hpp (tile_prologue,
//                        roll_window, the run finder, the heads and stitch kernels, run_scan).  It makes no table probe.
//
// The host makes the sites from the two run lists (gaps_host.hpp: stretches, kinds, a and q, the trims, edge and ragged), uploads them
// as they are and launches
//
//   gap_search_kernel    one wave per site, four per block, grid-stride, at most 1024 waves: a front search on the shared pieces of
//                        front_search.hpp.  F and G are front_flanks' (a non-base: the site is skipped).  Level t = 0,
//                        1, ..: the frontier S_t is at most GAP_FRONT = 64 strings, one per lane, but a lane keeps of its string y only
//                        W = the last k - 1 bases of F + y (128 bits) and the minimum over its windows.  The string itself is in the
//                        wave's LOG in global memory: row t - 1 holds 64 bytes, byte s = (the slot of S_(t-1) that slot s of S_t
//                        extends) << 2 | the base it adds.  The kernel's own part of each step:
//                          rejoin   (front_window0, front_rejoin with front_window) from W as it is.  A record's y is read out of the
//                                   log by its own lane, t rows back, and written as letters into the byte pool; the records and the
//                                   bytes of a level are front_reserve's two lists: all of both or nothing.  More than
//                                   GAP_MAX_RECORDS at a site: complex.
//                          close    t >= k - 1 and W == G: the string ends here (it is a record followed by the whole right flank).
//                          extend   (front_extend) strings that are closed have no children; the k-mer is W << 2 | z whatever t is,
//                                   since W always holds k - 1 bases.  W, the minimum and the log byte move through the strip, and
//                                   front_handover's lanes store the new row, 64 bytes side by side.
//                        Visibility of the log: a row is read only by lanes of the wave that stored it, later in program order.  The
//                        vector memory operations of one wave to global memory are performed in the order they were issued, and a CU's
//                        L1 serves the wave's loads behind its own write-through stores, so no cache has to be written back or dropped:
//                        the release / acquire fence pairs of WAVEFRONT scope of front_handover keep the compiler from moving the
//                        loads above the stores, which is all that is needed.  Nothing
//                        is handed between waves, and a later launch starts with clean caches.
//                        Every loop is bounded: levels <= max_len, rounds <= 4, the walk back <= t.  No spin; the only atomics are the
//                        cursor and counter adds.
//
// The record list starts at sites + 4096 entries and the byte pool at 2048 bytes per site to search + 16384; a search that wanted more of either has
// counted both and is repeated once with exactly that room (run_counted with its second list, scan_tile.hpp).  The dense scans are not repeated.
#include "gaps.hpp"
#include "front_search.hpp"

namespace jk {

enum { GC_BYTES = 1, GC_LOOKUPS = 2 };                                   // control words 1 and 2: pool bytes wanted; table lookups made

__device__ __forceinline__ uint32_t kind_of(GapRun) { return 1u; }
__device__ __forceinline__ GapRun absorb(GapRun r, GapRun p) {
    r.n_kmers += p.n_kmers;
    return r;
}

__global__ __launch_bounds__(RP_THREADS) void gap_runs_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                              uint64_t ntiles, int k, unsigned long long *__restrict__ counts, TileRuns *__restrict__ tout,
                                                              GapRun *__restrict__ part, unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + RP_HALO];
    __shared__ uint32_t s_mask[RP_THREADS];             // bit j of [g]: window w0 + 16g + j exists and has no k-mer
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_tot;
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t == 0) s_tot = 0;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc, h;
        int run;
        tile_prologue<RP_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        uint32_t im = 0;
#pragma unroll
        for (int j = 0; j < RP_GROUP; ++j) {
            const bool ok = roll_window(c, iv, j, k, kmask, 2 * k, e0, n, fwd, rc, run, h);
            im |= (!ok && e0 + j < n ? 1u : 0u) << j;
        }
        s_mask[t] = im;
        {
            const uint32_t ci = wave_sum((uint32_t)__popc(im));
            if (lane == 0 && ci) atomicAdd(&s_tot, ci);
        }
        __syncthreads();
        const uint32_t startmask = class_starts(im, s_mask);
        const TileSlots S = tile_reserve((uint32_t)__popc(startmask), s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0) tout[tile] = TileRuns{S.base0, S.total, tile_ends(s_mask)};
        if (t == 0 && s_tot) atomicAdd(&counts[D.seq], (unsigned long long)s_tot);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            uint32_t sm = startmask;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                GapRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = walk_run(s_mask, t * RP_GROUP + b0, [](int, int, int, int) {});
                r.seq = D.seq;
                r.pad = 0;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

// log: gridDim.x * 4 waves x max_len rows x GAP_FRONT bytes.  out has room for cap records and pool for pool_cap bytes.
__global__ __launch_bounds__(256) void gap_search_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, uint32_t n_seqs, TableDev R, uint32_t thre,
                                                         int max_len, GapSite *sites, uint64_t nsites, uint8_t *log, GapFill *__restrict__ out, unsigned long long cap,
                                                         uint8_t *__restrict__ pool, unsigned long long pool_cap, unsigned long long *__restrict__ ctl) {
    __shared__ ulonglong2 s_w[4][GAP_FRONT];            // a wave's next frontier: W (.x low, .y high) ...
    __shared__ uint32_t s_mn[4][GAP_FRONT];             // ... its running minimum ...
    __shared__ uint8_t s_b[4][GAP_FRONT];               // ... and its log byte
    const int lane = threadIdx.x & 63;
    ulonglong2 *strip_w = s_w[threadIdx.x >> 6];
    uint32_t *strip_mn = s_mn[threadIdx.x >> 6];
    uint8_t *strip_b = s_b[threadIdx.x >> 6];
    const int k = R.k;
    const u128 kmask = maskbits(2 * k), fmask = maskbits(2 * (k - 1));
    const uint64_t nwv = (uint64_t)gridDim.x * 4, wv = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint8_t *mylog = log + wv * (uint64_t)max_len * GAP_FRONT;
    unsigned long long nlook = 0;                       // (wave-uniform)
    for (uint64_t i = wv; i < nsites; i += nwv) {
        const GapSite S = sites[i];
        if (S.status >= GAP_EDGE || S.seq >= n_seqs) continue;      // (wave-uniform, like every check here) the host's own verdicts stay
        const int64_t o0 = offs[S.seq];
        const int64_t n = offs[S.seq + 1] - o0;
        const int64_t RL = S.q - S.a;
        if (S.a < k - 1 || RL < 0 || S.q > n - (k - 1)) continue;      // F and G lie inside the sequence (the host writes no other site)
        const Flanks FG = front_flanks(text + o0, S.a, S.q, k);
        uint32_t status = GAP_NONE, nrec = 0;
        int t = 0;
        if (!FG.bases) {
            status = GAP_SKIPPED;                       // ... and are bases
        } else {
            const u128 F = FG.F, G = FG.G;
            // level 0: S_0 = {empty}
            u128 W = F;                                 // lane i < nf: the last k - 1 bases of F + (string i) ...
            uint32_t mn = 0xFFFFFFFFu;                  // ... the minimum over its windows ...
            bool alive = lane == 0;                     // ... and whether it is (still) in S_t
            int nf = 1;
            for (;; ++t) {                              // (t <= max_len: the stop check)
                // rejoin: window t, lane i for string i
                uint32_t a = 0xFFFFFFFFu;
                if (alive) a = canon_count(R, front_window0(W, G, k, kmask), k);
                nlook += (unsigned)__popcll(__ballot(alive));
                a = min32(a, mn);
                uint32_t my_amin;
                const unsigned long long recm = front_rejoin(R, thre, __ballot(alive && a >= thre), a, nlook, my_amin, [&](int j) { return front_window(readlane128(W, j), G, k, kmask); });
                if (recm) {
                    const unsigned total = __popcll(recm);
                    if (nrec + total > (uint32_t)GAP_MAX_RECORDS) {      // the level lists none of them
                        status = GAP_COMPLEX;
                        break;
                    }
                    nrec += total;
                    unsigned long long off;             // the records and their t bytes each: all of the level in both lists or nothing
                    const unsigned long long at = front_reserve(recm, &ctl[SC_CURSOR], cap, &ctl[GC_BYTES], (unsigned)t, pool_cap, &off);
                    if (at != FRONT_NONE) {
                        int slot = lane;                // y, last base first: t rows back through the log (slot <= 63; rows 0 .. t - 1 < max_len)
                        for (int r = t; r >= 1; --r) {
                            const uint32_t b = mylog[(uint64_t)(r - 1) * GAP_FRONT + slot];
                            pool[off + (unsigned)(r - 1)] = (uint8_t)(0x54474341u >> (8 * (b & 3u)));
                            slot = (int)(b >> 2);
                        }
                        GapFill v;
                        v.pos = S.a;
                        v.bases_off = off;
                        v.seq = S.seq;
                        v.ref_len = (uint32_t)RL;
                        v.len = (uint32_t)t;
                        v.alt_min = my_amin;
                        out[at] = v;
                    }
                }
                // close: the string holds the whole right flank
                if (t >= k - 1 && alive && eq(W, G)) alive = false;
                const int nalive = __popcll(__ballot(alive));
                // stop check
                if (t >= max_len) {
                    status = nalive ? GAP_LIMIT : GAP_DEAD;
                    break;
                }
                if (nalive == 0) {
                    status = GAP_DEAD;
                    break;
                }
                // extend S_t to S_(t+1): sixteen strings a round, (string, z) on lane 4 * string + z
                const int tot = front_extend(
                    R, thre, W, mn, nf, GAP_FRONT,
                    [=](int src, u128 parent) {      // (by value: capturing `alive` by reference costs two VGPRs)
                        const u128 nw = band(bor(shl(parent, 2), mk(0, (uint64_t)(lane & 3))), kmask);      // the k-mer: W holds k - 1 bases
                        return FrontChild<u128>{band(nw, fmask), nw, __shfl((int)alive, src) != 0, true};
                    },
                    [&](int at, int src, u128 w1, uint32_t m) {
                        strip_w[at] = make_ulonglong2(w1.lo, w1.hi);
                        strip_mn[at] = m;
                        strip_b[at] = (uint8_t)((src << 2) | (lane & 3));
                    });
                nlook += 4u * (unsigned)nalive;
                if (tot > GAP_FRONT || tot == 0) {      // level t + 1 cannot be formed: complex, or nothing is left
                    status = tot ? GAP_COMPLEX : GAP_DEAD;
                    ++t;
                    break;
                }
                alive = lane < tot;
                front_handover(tot, [&](int l) {        // the row is read by whichever lane lists a record later on
                    const ulonglong2 v = strip_w[l];
                    W = mk(v.y, v.x);
                    mn = strip_mn[l];
                    mylog[(uint64_t)t * GAP_FRONT + l] = strip_b[l];      // row t = level t + 1  (t < max_len)
                });
                nf = tot;
            }
        }
        if (lane == 0) {
            sites[i].n_records = nrec;
            sites[i].levels = (uint32_t)t;
            sites[i].status = (uint8_t)status;
        }
    }
    if (lane == 0 && nlook) atomicAdd(&ctl[GC_LOOKUPS], nlook);
}

static int gap_check_args(const Table &T, uint32_t thre, int max_len, int64_t max_trim, std::string &err) {
    if (thre < 1) { err = "gap scan: the threshold (thre) must be at least 1"; return -1; }
    if (T.k < 2) { err = "gap scan: k must be at least 2"; return -1; }
    if (max_len < 0 || max_len > GAP_MAX_LEN) { err = "gap scan: max_len must be in 0..4096"; return -1; }
    if (max_trim < 0) { err = "gap scan: max_trim must be at least 0"; return -1; }
    return 0;
}

// the search on out.sites (in (seq, a) order; the host's verdicts edge and ragged are in), then the checks, the order and the counters
static int gap_search_sites(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, GapOut &out, std::string &err) {
    std::vector<GapSite> &sites = out.sites;
    const uint64_t nsites = sites.size();
    uint64_t nsearch = 0;
    for (const GapSite &S : sites) nsearch += S.status == GAP_NONE;
    if (nsearch) {                                      // (else nothing of the search is allocated or launched)
        hipStream_t st = T.stream;
        const int W = Table::WS_GAPS + 8;
        const unsigned grid = (unsigned)std::min<uint64_t>((nsearch + 3) / 4, 256);      // at most 1024 waves, each with a log of its own
        const size_t log_bytes = std::max<size_t>((size_t)grid * 4 * (size_t)max_len * GAP_FRONT, 64);
        GapSite *d_sites = (GapSite *)T.workspace(W, nsites * sizeof(GapSite), err);
        int64_t *d_offs = (int64_t *)T.workspace(W + 1, ((size_t)n_seqs + 1) * sizeof(int64_t), err);
        unsigned long long *d_ctl = (unsigned long long *)T.workspace(W + 2, SC_WORDS * sizeof(unsigned long long), err), ctl[SC_WORDS] = {0, 0, 0, 0};
        uint8_t *d_log = (uint8_t *)T.workspace(W + 3, log_bytes, err);
        if (!d_sites || !d_offs || !d_ctl || !d_log) return -1;
        HIPCHK(hipMemcpyAsync(d_sites, sites.data(), nsites * sizeof(GapSite), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_offs, offsets, ((size_t)n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        GapFill *d_rec = nullptr;
        uint8_t *d_pool = nullptr;
        unsigned long long pool_cap = 2048 * nsearch + 16384;
        auto search = [&](unsigned long long cap) {
            d_rec = (GapFill *)T.workspace(W + 4, cap * sizeof(GapFill), err);
            d_pool = (uint8_t *)T.workspace(W + 5, pool_cap, err);
            if (!d_rec || !d_pool) return -1;
            hipLaunchKernelGGL(gap_search_kernel, dim3(grid), dim3(256), 0, st, d_text, d_offs, (uint32_t)n_seqs, T.d, thre, max_len, d_sites, nsites, d_log, d_rec, cap, d_pool,
                               pool_cap, d_ctl);
            return 0;
        };
        if (run_counted(st, d_ctl, SC_WORDS, d_ctl, nsites + 4096, "gap scan: the number of records or of their bases changed between two searches", ctl, out.search_seconds,
                        out.retried, err, search, GC_BYTES, &pool_cap))
            return -1;
        out.seconds += out.search_seconds;
        out.lookups = ctl[GC_LOOKUPS];
        out.fills.resize(ctl[SC_CURSOR]);
        out.pool.resize(ctl[GC_BYTES]);
        HIPCHK(hipMemcpyAsync(sites.data(), d_sites, nsites * sizeof(GapSite), hipMemcpyDeviceToHost, st));
        if (!out.fills.empty()) HIPCHK(hipMemcpyAsync(out.fills.data(), d_rec, out.fills.size() * sizeof(GapFill), hipMemcpyDeviceToHost, st));
        if (!out.pool.empty()) HIPCHK(hipMemcpyAsync(out.pool.data(), d_pool, out.pool.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
    }
    if (gap_check_records(sites, out.fills, out.pool, thre, max_len, err)) return -1;
    const std::vector<char> &pool = out.pool;
    std::sort(out.fills.begin(), out.fills.end(), [&pool](const GapFill &a, const GapFill &b) {
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.len != b.len) return a.len < b.len;
        return a.len && std::memcmp(pool.data() + a.bases_off, pool.data() + b.bases_off, a.len) < 0;
    });
    std::vector<char> packed;                           // the bases in the records' order: the pool does not depend on the order of the cursor adds
    packed.reserve(pool.size());
    for (GapFill &v : out.fills) {
        const uint64_t off = packed.size();
        packed.insert(packed.end(), pool.begin() + (ptrdiff_t)v.bases_off, pool.begin() + (ptrdiff_t)(v.bases_off + v.len));
        v.bases_off = off;
    }
    out.pool.swap(packed);
    gap_counts(n_seqs, sites, out.counts);
    return 0;
}

int gap_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, int64_t max_trim, bool long_runs, ReportOut &report,
                    GapOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "gap scan: bad arguments"; return -1; }
    if (gap_check_args(T, thre, max_len, max_trim, err)) return -1;
    out = GapOut();
    if (kmer_report_device(T, n_seqs, d_text, offsets, thre, report, err)) return -1;
    out.seconds = report.seconds;
    std::vector<uint64_t> rcounts;
    std::vector<GapRun> inval;
    int runs_retried = 0;
    const int k = T.k;
    if (run_scan(T, Table::WS_GAPS, "gap scan", n_seqs, d_text, offsets, 1, 2, rcounts, inval, out.runs_seconds, runs_retried, err,
                 [&](unsigned grid, hipStream_t st, const TileList &L, uint64_t ntiles, unsigned long long *d_cnt, TileRuns *d_tout, GapRun *d_part, unsigned long long cap,
                     unsigned long long *d_ctl) {
                     hipLaunchKernelGGL(gap_runs_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, k, d_cnt, d_tout, d_part, cap, d_ctl);
                 }))
        return -1;
    out.seconds += out.runs_seconds;
    for (int i = 0; i < n_seqs; ++i) {                  // the two dense scans saw the same windows: every one is valid or in a run of this one
        if (rcounts[2 * (size_t)i] != report.counts[4 * (size_t)i] || rcounts[2 * (size_t)i + 1] + report.counts[4 * (size_t)i + 1] != report.counts[4 * (size_t)i]) {
            err = "gap scan: the windows without a k-mer and the valid windows do not add up";
            return -1;
        }
    }
    if (gap_build_sites(k, n_seqs, offsets, report.runs, inval, max_trim, long_runs, out.sites, err)) return -1;
    return gap_search_sites(T, n_seqs, d_text, offsets, thre, max_len, out, err);
}

int gap_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int64_t max_trim, bool long_runs, ReportOut &report,
                  GapOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "gap scan: bad arguments"; return -1; }
    if (gap_check_args(T, thre, max_len, max_trim, err)) return -1;
    HostText H;
    if (pack_host_text(T, Table::WS_REPORT, n_seqs, seqs, lens, "gap scan", H, err)) return -1;
    return gap_scan_device(T, n_seqs, H.d_text, H.offs.data(), thre, max_len, max_trim, long_runs, report, out, err);
}

int gap_search_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, const GapSite *sites, uint64_t n_sites, GapOut &out,
                      std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets) || (n_sites && !sites)) { err = "gap search: bad arguments"; return -1; }
    if (gap_check_args(T, thre, max_len, 0, err)) return -1;
    out = GapOut();
    out.sites.assign(sites, sites + n_sites);
    if (gap_check_sites(T.k, n_seqs, offsets, out.sites, err)) return -1;      // (a malformed list launches nothing)
    HIPCHK(hipSetDevice(T.device));
    if (T.materialize(err)) return -1;
    return gap_search_sites(T, n_seqs, d_text, offsets, thre, max_len, out, err);
}

int gap_search_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, const GapSite *sites, uint64_t n_sites, GapOut &out,
                    std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens)) || (n_sites && !sites)) { err = "gap search: bad arguments"; return -1; }
    if (gap_check_args(T, thre, max_len, 0, err)) return -1;
    {                                                   // the list is checked before anything is uploaded
        std::vector<GapSite> probe(sites, sites + n_sites);
        std::vector<int64_t> offs((size_t)n_seqs + 1, 0);
        for (int i = 0; i < n_seqs; ++i) offs[(size_t)i + 1] = offs[i] + lens[i];
        if (gap_check_sites(T.k, n_seqs, offs.data(), probe, err)) return -1;
    }
    HostText H;
    if (pack_host_text(T, Table::WS_REPORT, n_seqs, seqs, lens, "gap search", H, err)) return -1;
    return gap_search_device(T, n_seqs, H.d_text, H.offs.data(), thre, max_len, sites, n_sites, out, err);
}

}  // namespace jk
