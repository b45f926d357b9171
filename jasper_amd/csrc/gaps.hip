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
//   gap_search_kernel    one wave per site, four per block, grid-stride, at most 1024 waves.  F = the k - 1 bases before a and G = the
//                        k - 1 bases from q on are loaded and checked as compound_search_kernel does.  Then the bounded breadth-first
//                        search of jasper_gap_scan, level t = 0, 1, ..: the frontier S_t is at most GAP_FRONT = 64 strings, one per
//                        lane, but a lane keeps of its string y only W = the last k - 1 bases of F + y (128 bits) and the minimum over
//                        its windows.  The string itself is in the wave's LOG in global memory: row t - 1 holds 64 bytes, byte s =
//                        (the slot of S_(t-1) that slot s of S_t extends) << 2 | the base it adds.
//                          rejoin   window t of F + y + G, lane i for its own string, from W and G's first base; then, per string that
//                                   passed, lane j cuts window t + 1 + j out of W and G  (k - 2 lookups), as the compound search does.
//                                   A record's y is read out of the log by its own lane, t rows back, and written as letters into the
//                                   byte pool; the records and the bytes of a level take one returning cursor add each, and a level
//                                   writes all of both or nothing.  More than GAP_MAX_RECORDS at a site: complex.
//                          close    t >= k - 1 and W == G: the string ends here (it is a record followed by the whole right flank).
//                          extend   (string, z) on lane 4 * string + z, sixteen strings a round: the k-mer is W << 2 | z whatever t is,
//                                   since W always holds k - 1 bases.  A child's place is a popcount of the round's ballot; W, the
//                                   minimum and the log byte move through a per-wave LDS strip, and the new row is stored by the lanes
//                                   that take the children over, 64 bytes side by side.
//                        Visibility of the log: a row is read only by lanes of the wave that stored it, later in program order.  The
//                        vector memory operations of one wave to global memory are performed in the order they were issued, and a CU's
//                        L1 serves the wave's loads behind its own write-through stores, so no cache has to be written back or dropped:
//                        a release / acquire fence pair of WAVEFRONT scope around the hand-over keeps the compiler from moving the
//                        loads above the stores, which is all that is needed (the form compound.hip uses for its LDS strip).  Nothing
//                        is handed between waves, and a later launch starts with clean caches.
//                        Every loop is bounded: levels <= max_len, rounds <= 4, the walk back <= t.  No spin; the only atomics are the
//                        cursor and counter adds.
//
// The record list starts at sites + 4096 entries and the byte pool at 2048 bytes per site to search + 16384; a search that wanted more of either has
// counted both and is repeated once with exactly that room (counted_twice, beside run_counted's rule).  The dense scans are not repeated.
#include "gaps.hpp"
#include "scan_tile.hpp"

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

__device__ __forceinline__ uint32_t gp_count(const TableDev &R, u128 fwd, int k) {
    const u128 rc = revcomp(fwd, k);
    return clamp32(table_get(R, mix(lt(rc, fwd) ? rc : fwd, R.B)));
}
__device__ __forceinline__ uint32_t gp_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
__device__ __forceinline__ uint64_t gp_or64(uint64_t v) {      // OR over the wave, in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t gp_readlane64(uint64_t v, int l) {      // l wave-uniform
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t gp_first64(uint64_t v) {      // a value all lanes hold, as a scalar
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
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
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint64_t nwv = (uint64_t)gridDim.x * 4, wv = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint8_t *mylog = log + wv * (uint64_t)max_len * GAP_FRONT;
    unsigned long long nlook = 0;                       // (wave-uniform)
    for (uint64_t i = wv; i < nsites; i += nwv) {
        const GapSite S = sites[i];
        if (S.status >= GAP_EDGE || S.seq >= n_seqs) continue;      // (wave-uniform, like every check here) the host's own verdicts stay
        const int64_t o0 = offs[S.seq];
        const int64_t n = offs[S.seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        const int64_t RL = S.q - S.a;
        if (S.a < k - 1 || RL < 0 || S.q > n - (k - 1)) continue;      // F and G lie inside the sequence (the host writes no other site)
        int cf = 0, cg = 0;
        if (lane < k - 1) {
            cf = code(txt[S.a - (k - 1) + lane]);
            cg = code(txt[S.q + lane]);
        }
        uint32_t status = GAP_NONE, nrec = 0;
        int t = 0;
        if (__ballot(cf < 0 || cg < 0)) {
            status = GAP_SKIPPED;                       // ... and are bases
        } else {
            const unsigned sh = lane < k - 1 ? 2u * (unsigned)(k - 2 - lane) : 0u;      // base l of F and of G: bit pair k - 2 - l
            const u128 f1 = lane < k - 1 ? shl(mk(0, (uint64_t)cf), sh) : mk(0, 0), g1 = lane < k - 1 ? shl(mk(0, (uint64_t)cg), sh) : mk(0, 0);
            const u128 F = mk(gp_first64(gp_or64(f1.hi)), gp_first64(gp_or64(f1.lo))), G = mk(gp_first64(gp_or64(g1.hi)), gp_first64(gp_or64(g1.lo)));
            // level 0: S_0 = {empty}
            u128 W = F;                                 // lane i < nf: the last k - 1 bases of F + (string i) ...
            uint32_t mn = 0xFFFFFFFFu;                  // ... the minimum over its windows ...
            bool alive = lane == 0;                     // ... and whether it is (still) in S_t
            int nf = 1;
            for (;; ++t) {                              // (t <= max_len: the stop check)
                // rejoin: window t, lane i for string i
                uint32_t a = 0xFFFFFFFFu;
                if (alive) a = gp_count(R, band(bor(shl(W, 2), shr(G, 2 * (k - 2))), kmask), k);
                nlook += (unsigned)__popcll(__ballot(alive));
                a = gp_min(a, mn);
                const unsigned long long P = __ballot(alive && a >= thre);
                unsigned long long recm = 0;            // (wave-uniform) bit i: string i is a record
                uint32_t my_amin = a;
                if (k > 2) {
                    for (unsigned long long p = P; p; p &= p - 1ull) {
                        const int j = (int)__builtin_ctzll(p);
                        const u128 Wj = mk(gp_readlane64(W.hi, j), gp_readlane64(W.lo, j));
                        const uint32_t aj = (uint32_t)__builtin_amdgcn_readlane((int)a, j);
                        uint32_t b = 0xFFFFFFFFu;
                        if (lane < k - 2)               // window t + 1 + lane: the last k - 2 - lane bases of W, then lane + 2 bases of G
                            b = gp_count(R, band(bor(shl(Wj, 2 * (lane + 2)), shr(G, 2 * (k - 3 - lane))), kmask), k);
                        nlook += (unsigned)(k - 2);
                        b = gp_min(wave_min32(b), aj);
                        if (b >= thre) {
                            recm |= 1ull << j;
                            if (lane == j) my_amin = b;
                        }
                    }
                } else {
                    recm = P;
                }
                if (recm) {
                    const unsigned total = __popcll(recm);
                    if (nrec + total > (uint32_t)GAP_MAX_RECORDS) {      // the level lists none of them
                        status = GAP_COMPLEX;
                        break;
                    }
                    nrec += total;
                    unsigned long long base = 0, bbase = 0;
                    if (lane == 0) {
                        base = atomicAdd(&ctl[SC_CURSOR], (unsigned long long)total);
                        bbase = atomicAdd(&ctl[GC_BYTES], (unsigned long long)total * (unsigned)t);
                    }
                    base = __shfl(base, 0);
                    bbase = __shfl(bbase, 0);
                    if (base + total <= cap && bbase + (unsigned long long)total * (unsigned)t <= pool_cap && ((recm >> lane) & 1ull)) {      // (all of the level or nothing)
                        const unsigned mine = __popcll(recm & below);
                        const unsigned long long off = bbase + (unsigned long long)mine * (unsigned)t;
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
                        out[base + mine] = v;
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
                int tot = 0;
                for (int r0 = 0; r0 < nf; r0 += 16) {
                    const int src = r0 + (lane >> 2);   // <= 63
                    const u128 nw = band(bor(shl(mk(__shfl(W.hi, src), __shfl(W.lo, src)), 2), mk(0, (uint64_t)(lane & 3))), kmask);      // the k-mer: W holds k - 1 bases
                    const uint32_t pm = (uint32_t)__shfl(mn, src);
                    const bool from = __shfl((int)alive, src) != 0 && src < nf;
                    uint32_t c = 0;
                    if (from) c = gp_count(R, nw, k);
                    const bool ok = from && c >= thre;
                    const unsigned long long B = __ballot(ok);
                    const int at = tot + __popcll(B & below);
                    if (ok && at < GAP_FRONT) {
                        const u128 w1 = band(nw, fmask);
                        strip_w[at] = make_ulonglong2(w1.lo, w1.hi);
                        strip_mn[at] = gp_min(pm, c);
                        strip_b[at] = (uint8_t)((src << 2) | (lane & 3));
                    }
                    tot += __popcll(B);
                }
                nlook += 4u * (unsigned)nalive;
                if (tot > GAP_FRONT || tot == 0) {      // level t + 1 cannot be formed: complex, or nothing is left
                    status = tot ? GAP_COMPLEX : GAP_DEAD;
                    ++t;
                    break;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                alive = lane < tot;
                if (alive) {
                    const ulonglong2 v = strip_w[lane];
                    W = mk(v.y, v.x);
                    mn = strip_mn[lane];
                    mylog[(uint64_t)t * GAP_FRONT + lane] = strip_b[lane];      // row t = level t + 1  (t < max_len)
                }
                // the strip may be written again, and the row is read by whichever lane lists a record later on
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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

// run_counted's rule for a kernel that appends to TWO lists: launch(cap, pool_cap) sizes both and launches on st; the kernel adds what it
// WANTED to ctl[SC_CURSOR] (records) and ctl[GC_BYTES] (pool bytes) and writes nothing of a level that does not fit both.  If more of
// either was wanted, it is repeated once with exactly that room; more still is an error.
template <class Launch>
static int counted_twice(hipStream_t st, unsigned long long *d_ctl, unsigned long long cap, unsigned long long pool_cap, unsigned long long (&ctl)[SC_WORDS], double &seconds,
                         int &retried, std::string &err, Launch &&launch) {
    Events ev;
    if (ev.create(err)) return -1;
    for (int attempt = 0;; ++attempt) {
        HIPCHK(hipMemsetAsync(d_ctl, 0, SC_WORDS * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        if (launch(cap, pool_cap)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        if (ev.add_seconds(seconds, err)) return -1;
        if (ctl[SC_CURSOR] <= cap && ctl[GC_BYTES] <= pool_cap) return 0;
        if (attempt) { err = "gap scan: the number of records or of their bases changed between two searches"; return -1; }
        cap = std::max(cap, ctl[SC_CURSOR]);            // the kernel counted what it could not write: exactly this much room is needed
        pool_cap = std::max(pool_cap, ctl[GC_BYTES]);
        retried = 1;
    }
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
        auto search = [&](unsigned long long cap, unsigned long long pool_cap) {
            d_rec = (GapFill *)T.workspace(W + 4, cap * sizeof(GapFill), err);
            d_pool = (uint8_t *)T.workspace(W + 5, pool_cap, err);
            if (!d_rec || !d_pool) return -1;
            hipLaunchKernelGGL(gap_search_kernel, dim3(grid), dim3(256), 0, st, d_text, d_offs, (uint32_t)n_seqs, T.d, thre, max_len, d_sites, nsites, d_log, d_rec, cap, d_pool,
                               pool_cap, d_ctl);
            return 0;
        };
        if (counted_twice(st, d_ctl, nsites + 4096, 2048 * nsearch + 16384, ctl, out.search_seconds, out.retried, err, search)) return -1;
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
