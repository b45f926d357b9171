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
//   report_heads_kernel   one workgroup: a partial run is the HEAD of a final run unless it continues the last partial run of the
//                         tile before it (same sequence, open on both sides); exclusive sum of heads per tile = where a tile's
//                         final runs go.  Tiles are in (sequence, position) order, so the final list is too, whatever order
//                         the tiles' cursor adds happened in.
//   report_stitch_kernel  one wave per tile: each head is copied to its final place; the head that is open at its tile's end first
//                         absorbs the continuing partial runs of the tiles after it (sums and min).
//
// The number of runs is not known before the scan: the list of partial runs starts at windows / 64 + 64K entries (half a byte per
// window); a scan that needed more has counted how many, and is repeated once with exactly that room.
#include "report.hpp"
#include <algorithm>
#include <cstring>

namespace jk {

#define HIPCHK(x)                                                                     \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            err = std::string(#x) + ": " + hipGetErrorString(e_);                     \
            return -1;                                                                \
        }                                                                             \
    } while (0)

struct RpTile { uint32_t seq, idx; };                                    // tile idx (windows idx * RP_TILE ..) of sequence seq
struct RpTileOut { unsigned long long base; uint32_t nruns, flags; };    // its partial runs: part[base .. base + nruns)
enum { RP_OPEN_START = 1, RP_OPEN_END = 2 };                             // the tile's first / last window is unreliable
enum { RC_CURSOR = 0, RC_HEADS = 1, RC_WORDS = 4 };                      // control words: partial runs wanted, final runs

__device__ __forceinline__ uint32_t wave_incl_scan32(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(RP_THREADS) void report_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const RpTile *__restrict__ tiles,
                                                                 uint64_t ntiles, TableDev T, uint32_t thre, unsigned long long *__restrict__ counts,
                                                                 RpTileOut *__restrict__ tout, KmerRun *__restrict__ part, unsigned long long cap,
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
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k = T.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const RpTile D = tiles[tile];
        const int64_t o0 = offs[D.seq];
        const int64_t n = offs[D.seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        const int64_t w0 = (int64_t)D.idx * RP_TILE;    // the tile's first window
        const int64_t origin = w0 + k - 1;              // ... ends here
        if (t < 3) s_tot[t] = 0;
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
        uint32_t vm = 0, um = 0, am = 0, gmin = 0xFFFFFFFFu;
#pragma unroll
        for (int j0 = 0; j0 < RP_GROUP; j0 += 4) {
            u128 hs[4];
            bool ok[4];
            ulonglong2 ent[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                const uint32_t cj = (c >> (30 - 2 * j)) & 3u;
                const bool bad = (iv >> (15 - j)) & 1u;
                fwd = band(bor(shl(fwd, 2), mk(0, cj)), kmask);
                rc = bor(shr(rc, 2), shl(mk(0, 3u - cj), 2 * (k - 1)));
                run = bad ? 0 : run + 1;
                ok[u] = run >= k && e0 + j < n;
                hs[u] = mix(lt(rc, fwd) ? rc : fwd, T.B);
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
            const uint32_t cv = wave_sum32(__popc(vm)), cu = wave_sum32(__popc(um)), ca = wave_sum32(__popc(am));
            if (lane == 0) {
                atomicAdd(&s_tot[0], cv);
                atomicAdd(&s_tot[1], cu);
                atomicAdd(&s_tot[2], ca);
            }
        }
        __syncthreads();
        // where my runs start: an unreliable window after one that is not (the tile's first window starts one anyway)
        const uint32_t carry = t > 0 ? (s_unrel[t - 1] >> 15) & 1u : 0u;
        const uint32_t startmask = um & ~((um << 1) | carry) & 0xFFFFu;
        const uint32_t ns = __popc(startmask);
        const uint32_t incl = wave_incl_scan32(ns);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RP_THREADS / 64; ++w) {
            woff += w < wave ? s_wsum[w] : 0u;
            total += s_wsum[w];
        }
        if (t == 0) {
            const unsigned long long b = total ? atomicAdd(&ctl[RC_CURSOR], (unsigned long long)total) : 0ull;
            s_base = b;
            RpTileOut O;
            O.base = b;
            O.nruns = total;
            O.flags = ((s_unrel[0] & 1u) ? RP_OPEN_START : 0) | (((s_unrel[RP_THREADS - 1] >> 15) & 1u) ? RP_OPEN_END : 0);
            tout[tile] = O;
        }
        if (t < 3 && s_tot[t]) atomicAdd(&counts[3ull * D.seq + t], (unsigned long long)s_tot[t]);
        __syncthreads();
        const unsigned long long base = s_base;
        if (base + total <= cap) {
            uint32_t sm = startmask;
            unsigned long long at = base + woff + incl - ns;
            while (sm) {
                const int b0 = __builtin_ctz(sm);
                sm &= sm - 1;
                int pos = t * RP_GROUP + b0;
                uint64_t nk = 0, na = 0;
                uint32_t mn = 0xFFFFFFFFu;
                while (pos < RP_TILE) {
                    const int g = pos >> 4, b = pos & 15;
                    const uint32_t U = s_unrel[g] >> b;
                    const int len = __builtin_ctz(~U);            // (bits 16.. of U are clear: len <= 16 - b)
                    if (len == 0) break;
                    if (len == RP_GROUP) mn = min(mn, s_gmin[g]);
                    else
                        for (int j = 0; j < len; ++j) mn = min(mn, s_cnt[pos + j]);
                    na += __popc((s_abs[g] >> b) & ((1u << len) - 1u));
                    nk += len;
                    pos += len;
                    if (b + len < RP_GROUP) break;
                }
                KmerRun r;
                r.start = w0 + t * RP_GROUP + b0;
                r.n_kmers = nk;
                r.n_absent = na;
                r.seq = D.seq;
                r.min_count = mn;
                part[at++] = r;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

// 1 if the first partial run of tile i continues the last one of tile i - 1
__device__ __forceinline__ uint32_t rp_cont(const RpTile *__restrict__ tiles, const RpTileOut *__restrict__ tout, uint64_t i) {
    if (i == 0 || tiles[i].idx == 0) return 0u;         // (idx > 0: tile i - 1 is the tile before it in the same sequence)
    return (tout[i].flags & RP_OPEN_START) && (tout[i - 1].flags & RP_OPEN_END) ? 1u : 0u;
}

constexpr int RH_THREADS = 1024;
__global__ __launch_bounds__(RH_THREADS) void report_heads_kernel(const RpTile *__restrict__ tiles, const RpTileOut *__restrict__ tout, uint64_t ntiles,
                                                                  unsigned long long *__restrict__ head_base, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_w[RH_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t per = (ntiles + RH_THREADS - 1) / RH_THREADS;
    const uint64_t lo = (uint64_t)t * per < ntiles ? (uint64_t)t * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    unsigned long long sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += tout[i].nruns - rp_cont(tiles, tout, i);
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
        at += tout[i].nruns - rp_cont(tiles, tout, i);
    }
    if (t == RH_THREADS - 1) ctl[RC_HEADS] = at;
}

__global__ __launch_bounds__(256) void report_stitch_kernel(const RpTile *__restrict__ tiles, const RpTileOut *__restrict__ tout,
                                                            const unsigned long long *__restrict__ head_base, uint64_t ntiles, const KmerRun *__restrict__ part,
                                                            KmerRun *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ntiles; i += nwv) {
        const RpTileOut O = tout[i];
        const uint32_t cont = rp_cont(tiles, tout, i);
        for (uint32_t j = lane + cont; j < O.nruns; j += 64) {
            KmerRun r = part[O.base + j];
            if (j == O.nruns - 1 && (O.flags & RP_OPEN_END)) {
                for (uint64_t q = i + 1; q < ntiles && tiles[q].idx != 0; ++q) {
                    const RpTileOut Q = tout[q];
                    if (!(Q.flags & RP_OPEN_START)) break;
                    const KmerRun p = part[Q.base];
                    r.n_kmers += p.n_kmers;
                    r.n_absent += p.n_absent;
                    r.min_count = min(r.min_count, p.min_count);
                    if (Q.nruns != 1 || !(Q.flags & RP_OPEN_END)) break;      // that run ends inside tile q
                }
            }
            out[head_base[i] + j - cont] = r;
        }
    }
}

namespace {
struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

int kmer_report_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, ReportOut &R, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "kmer report: bad arguments"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    if (T.materialize(err)) return -1;
    const int k = T.k;
    R.counts.assign((size_t)n_seqs * 4, 0);
    R.runs.clear();
    R.seconds = 0;
    R.retried = 0;
    std::vector<RpTile> tiles;
    uint64_t windows = 0;
    for (int i = 0; i < n_seqs; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0) { err = "kmer report: offsets must not decrease"; return -1; }
        const int64_t n = offsets[i + 1] - offsets[i];
        const uint64_t w = n >= k ? (uint64_t)(n - k + 1) : 0;
        R.counts[4 * (size_t)i] = w;
        windows += w;
        const uint64_t nt = (w + RP_TILE - 1) / RP_TILE;
        if (nt > 0xFFFFFFFFull) { err = "kmer report: sequence too long"; return -1; }
        for (uint64_t q = 0; q < nt; ++q) tiles.push_back(RpTile{(uint32_t)i, (uint32_t)q});
    }
    const uint64_t ntiles = tiles.size();
    if (ntiles == 0) return 0;
    if (!d_text) { err = "kmer report: null text"; return -1; }
    hipStream_t st = T.stream;
    const int W = Table::WS_REPORT;
    int64_t *d_offs = (int64_t *)T.workspace(W + 1, ((size_t)n_seqs + 1) * sizeof(int64_t), err);
    RpTile *d_tiles = (RpTile *)T.workspace(W + 2, ntiles * sizeof(RpTile), err);
    RpTileOut *d_tout = (RpTileOut *)T.workspace(W + 3, ntiles * sizeof(RpTileOut), err);
    unsigned long long *d_head = (unsigned long long *)T.workspace(W + 4, ntiles * sizeof(unsigned long long), err);
    const size_t cnt_words = (size_t)n_seqs * 3 + RC_WORDS;
    unsigned long long *d_cnt = (unsigned long long *)T.workspace(W + 5, cnt_words * sizeof(unsigned long long), err);
    if (!d_offs || !d_tiles || !d_tout || !d_head || !d_cnt) return -1;
    unsigned long long *d_ctl = d_cnt + (size_t)n_seqs * 3;
    Events ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipMemcpyAsync(d_offs, offsets, ((size_t)n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), ntiles * sizeof(RpTile), hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 256 * 8);
    unsigned long long cap = windows / 64 + 65536, ctl[RC_WORDS] = {0, 0, 0, 0};
    KmerRun *d_part = nullptr;
    for (int attempt = 0;; ++attempt) {
        d_part = (KmerRun *)T.workspace(W + 6, cap * sizeof(KmerRun), err);
        if (!d_part) return -1;
        HIPCHK(hipMemsetAsync(d_cnt, 0, cnt_words * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(report_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, d_offs, d_tiles, ntiles, T.d, thre, d_cnt, d_tout, d_part, cap, d_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        R.seconds += ms * 1e-3;
        if (ctl[RC_CURSOR] <= cap) break;
        if (attempt) { err = "kmer report: the number of partial runs changed between two scans"; return -1; }
        cap = ctl[RC_CURSOR];            // the scan counted what it could not write: exactly this much room is needed
        R.retried = 1;
    }
    const uint64_t nparts = ctl[RC_CURSOR];
    std::vector<unsigned long long> cnt((size_t)n_seqs * 3);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (nparts) {
        KmerRun *d_out = (KmerRun *)T.workspace(W + 7, nparts * sizeof(KmerRun), err);
        if (!d_out) return -1;
        HIPCHK(hipEventRecord(ev.e[2], st));
        hipLaunchKernelGGL(report_heads_kernel, dim3(1), dim3(RH_THREADS), 0, st, d_tiles, d_tout, ntiles, d_head, d_ctl);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(report_stitch_kernel, dim3((unsigned)std::min<uint64_t>((ntiles + 3) / 4, 256 * 16)), dim3(256), 0, st, d_tiles, d_tout, d_head, ntiles, d_part,
                           d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[3], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
        R.seconds += ms * 1e-3;
        const uint64_t nruns = ctl[RC_HEADS];
        if (nruns > nparts) { err = "kmer report: more runs than partial runs"; return -1; }
        R.runs.resize(nruns);
        if (nruns) HIPCHK(hipMemcpyAsync(R.runs.data(), d_out, nruns * sizeof(KmerRun), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(jk_stream_wait(st));
    for (int i = 0; i < n_seqs; ++i)
        for (int c = 0; c < 3; ++c) R.counts[4 * (size_t)i + 1 + c] = cnt[3 * (size_t)i + c];
    return 0;
}

int kmer_report_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, ReportOut &R, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "kmer report: bad arguments"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    std::vector<int64_t> offs((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        if (lens[i] < 0 || (lens[i] && !seqs[i])) { err = "kmer report: bad sequence"; return -1; }
        offs[i + 1] = offs[i] + lens[i];
    }
    const size_t total = (size_t)offs[n_seqs];
    uint8_t *d_text = (uint8_t *)T.workspace(Table::WS_REPORT, total + 16, err);
    if (!d_text) return -1;
    if (n_seqs == 1) {
        if (total) HIPCHK(hipMemcpyAsync(d_text, seqs[0], total, hipMemcpyHostToDevice, T.stream));
        return kmer_report_device(T, n_seqs, d_text, offs.data(), thre, R, err);
    }
    std::vector<char> all(total);      // one copy for many short sequences; it lives until the report's last wait has returned
    for (int i = 0; i < n_seqs; ++i)
        if (lens[i]) memcpy(all.data() + offs[i], seqs[i], (size_t)lens[i]);
    if (total) HIPCHK(hipMemcpyAsync(d_text, all.data(), total, hipMemcpyHostToDevice, T.stream));
    return kmer_report_device(T, n_seqs, d_text, offs.data(), thre, R, err);
}

}  // namespace jk
