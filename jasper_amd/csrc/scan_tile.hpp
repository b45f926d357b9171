// scan_tile.hpp -- what the dense scans (report.hip, copies.hip, hapmers.hip, variants.hip and, through the last, indels.hip) have in
// common: everything before and after a scan kernel's probe loads, the two kernels that stitch partial runs, and the host stage around them.
//
// Device side.  A tile is RP_TILE windows of ONE sequence; thread t owns the 16 windows that end at origin + 16t ...
//   tile_prologue<HALO>   the tile and HALO groups of 16 bases before it staged into LDS (stage16), one barrier, and the thread's rolling
//                         state before its first window.  The report, the copy and the hap-mer scan look 64 bases back (RP_HALO), the
//                         variant scan 128 (VS_HALO): a run of 2k - 1 bases has to be seen.
//   roll_window           one window of the probe loop of a RUN scan: the rolling k-mer, its hash, and whether there is a k-mer at all.
//                         What a kernel loads and resolves for it is the kernel's own.
//   tile_reserve, tile_granted   from a thread's item count to its first place in the scan's global list: a block-wide exclusive sum, ONE
//                         cursor add per tile, and the rule that a tile writes all its items or none (the cursor has counted them either
//                         way, so the host can repeat the scan with exactly that room).  One barrier each; the kernel's own per-tile
//                         bookkeeping goes between the two.
//   class_starts, tile_ends, tile_ends2, walk_run   the run finder of a run scan.  A class is a 16-bit mask per thread in LDS; a run starts
//                         where a class bit follows a window without it (the thread before's bit 15 carries over; the tile's first window
//                         starts one anyway), and every start walks its class's masks to the run's or the tile's end, handing each piece
//                         inside one group to the kernel's own accumulation.
//   TileRuns              what a tile of a RUN scan leaves: where its partial runs are and the class of its first and last window.
//   scan_heads_kernel     one workgroup: a partial run is the HEAD of a final run unless it continues the last partial run of the tile
//                         before it (tile_continues); exclusive sum of heads per tile = where a tile's final runs go.  Tiles are in
//                         (sequence, position) order, so the final list is too, whatever order the tiles' cursor adds happened in.
//   scan_stitch_kernel    one wave per tile: each head is copied to its final place; the head that holds its tile's last window first
//                         absorbs the continuing partial runs of its kind of the tiles after it.  The run type brings two overloads:
//                         Run absorb(Run, Run) and kind_of(Run), by value (by reference costs the CopyRun kernel two VGPRs).
// Host side: pack_host_text (sequences in host memory -> one device text), settle (the tables of a scan zeroed and ordered before one
// stream), build_tiles / upload_tiles, run_counted (launch, read the control words, repeat once with exactly the counted room), stitch_runs,
// and run_scan, the whole host stage of a run scan around the caller's one kernel launch.  The workspace base stays the caller's: each scan
// has its own slots.  search_stage is the same for the front searches (front_search.hpp): control and per-sequence words, run_counted, the
// downloads and the add-up check around the caller's one kernel launch.
// Wave helpers, once: wave_incl_scan, wave_sum, wave_min32, wave_prefix_min32, min32, wave_or64, readlane64 / 128, readfirstlane64, and
// canon_count, a forward k-mer's count in a table.
#pragma once
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

struct ScanTile { uint32_t seq, idx; };                                  // tile idx (windows idx * RP_TILE ..) of sequence seq
struct TileRuns { unsigned long long base; uint32_t nruns, ends; };      // its partial runs: part[base .. base + nruns); ends = first class | last class << 2
enum { SC_CURSOR = 0, SC_HEADS = 1, SC_WORDS = 4 };                      // control words: items wanted; word 1 is the scan's own (final runs for a run scan)

__device__ __forceinline__ uint32_t ends_first(uint32_t ends) { return ends & 3u; }
__device__ __forceinline__ uint32_t ends_last(uint32_t ends) { return (ends >> 2) & 3u; }

template <class V> __device__ __forceinline__ V wave_incl_scan(V v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
template <class V> __device__ __forceinline__ V wave_sum(V v) {          // 32 or 64 bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t min32(uint32_t a, uint32_t b) { return b < a ? b : a; }
__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {              // OR over the wave, in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {      // l wave-uniform
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ u128 readlane128(u128 v, int l) { return mk(readlane64(v.hi, l), readlane64(v.lo, l)); }
__device__ __forceinline__ uint64_t readfirstlane64(uint64_t v) {        // a value all lanes hold, as a scalar
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// the table's count of the canonical form of the forward k-mer fwd, clamped to 32 bits
__device__ __forceinline__ uint32_t canon_count(const TableDev &R, u128 fwd, int k) {
    const u128 rc = revcomp(fwd, k);
    return clamp32(table_get(R, mix(lt(rc, fwd) ? rc : fwd, R.B)));
}

template <int N> __device__ __forceinline__ uint32_t wave_prefix_min32(uint32_t v) {      // lane j < N: the minimum over lanes 0 .. j
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < N; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v = u < v ? u : v;
    }
    return v;
}

// Tile D of the text: n = its sequence's length, w0 = the tile's first window, e0 = where my first window ends, (c, iv) = my 16 bases
// (stage16), fwd / rc = the k-mer that ends right before e0, run = bases in a row that end there (up to 16 * HALO).  s_code / s_inv hold
// RP_THREADS + HALO words.  Every thread of the block calls it; it holds one barrier.
template <int HALO>
__device__ __forceinline__ void tile_prologue(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, ScanTile D, int k, u128 kmask, uint32_t *s_code,
                                              uint32_t *s_inv, int64_t &n, int64_t &w0, int64_t &e0, uint32_t &c, uint32_t &iv, u128 &fwd, u128 &rc, int &run) {
    static_assert(HALO == 4 || HALO == 8, "the k-mer before a thread's first base is four groups; a halo of eight looks four further back");
    const int t = threadIdx.x;
    const int64_t o0 = offs[D.seq];
    n = offs[D.seq + 1] - o0;
    const uint8_t *__restrict__ txt = text + o0;
    w0 = (int64_t)D.idx * RP_TILE;
    const int64_t origin = w0 + k - 1;                  // the tile's first window ends here
    e0 = origin + (int64_t)t * RP_GROUP;
    stage16(txt, e0, n, c, iv);
    s_code[t + HALO] = c;
    s_inv[t + HALO] = iv;
    if (t < HALO) {
        uint32_t hc, hiv;
        stage16(txt, origin - (int64_t)(HALO - t) * RP_GROUP, n, hc, hiv);
        s_code[t] = hc;
        s_inv[t] = hiv;
    }
    __syncthreads();
    const uint32_t *pc = s_code + t + HALO - 4, *pi = s_inv + t + HALO - 4;      // the four groups before mine
    const uint64_t ivprev = ((uint64_t)pi[0] << 48) | ((uint64_t)pi[1] << 32) | ((uint64_t)pi[2] << 16) | (uint64_t)pi[3];
    fwd = band(mk(((uint64_t)pc[0] << 32) | pc[1], ((uint64_t)pc[2] << 32) | pc[3]), kmask);
    rc = revcomp(fwd, k);
    run = ivprev ? (int)__builtin_ctzll(ivprev) : 64;
    if (HALO == 8 && !ivprev) {
        const uint64_t ivfar = ((uint64_t)s_inv[t] << 48) | ((uint64_t)s_inv[t + 1] << 32) | ((uint64_t)s_inv[t + 2] << 16) | (uint64_t)s_inv[t + 3];
        run += ivfar ? (int)__builtin_ctzll(ivfar) : 64;
    }
}

// Window j (0 .. 15) of my 16: (c, iv) are my bases (stage16), e0 is where window 0 ends, n the sequence's length.  Rolls fwd / rc / run by
// one base, leaves the canonical k-mer's hash in h (B = 2k: the hash does not depend on a table's size) and says whether the window has a
// k-mer.
__device__ __forceinline__ bool roll_window(uint32_t c, uint32_t iv, int j, int k, u128 kmask, int B, int64_t e0, int64_t n, u128 &fwd, u128 &rc, int &run, u128 &h) {
    const uint32_t cj = (c >> (30 - 2 * j)) & 3u;
    const bool bad = (iv >> (15 - j)) & 1u;
    fwd = band(bor(shl(fwd, 2), mk(0, cj)), kmask);
    rc = bor(shr(rc, 2), shl(mk(0, 3u - cj), 2 * (k - 1)));
    run = bad ? 0 : run + 1;
    h = mix(lt(rc, fwd) ? rc : fwd, B);
    return run >= k && e0 + j < n;
}

// A thread's ns items of the tile: `first` is its first place among the tile's `total`.  Thread 0 adds total to *cursor and leaves the tile's
// place in the global list in *s_base (base0 is that place, in thread 0 only).  s_wsum holds RP_THREADS / 64 words.  One barrier.
struct TileSlots { uint32_t first, total; unsigned long long base0; };
__device__ __forceinline__ TileSlots tile_reserve(uint32_t ns, uint32_t *s_wsum, unsigned long long *s_base, unsigned long long *__restrict__ cursor) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t incl = wave_incl_scan(ns);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RP_THREADS / 64; ++w) {
        woff += w < wave ? s_wsum[w] : 0u;
        total += s_wsum[w];
    }
    TileSlots S = {woff + incl - ns, total, 0ull};
    if (t == 0) *s_base = S.base0 = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
    return S;
}
// ... and after one more barrier: may the tile write?  All its items or none: a list of cap entries has room for every one of them or the
// host repeats the scan.  `at` = my first place in the global list.
__device__ __forceinline__ bool tile_granted(TileSlots S, const unsigned long long *s_base, unsigned long long cap, unsigned long long &at) {
    __syncthreads();
    const unsigned long long base = *s_base;
    at = base + S.first;
    return base + S.total <= cap;
}

// ---- the run finder: s_mask[g] bit j = window 16g + j of the tile has the class; every thread's word is written and a barrier has passed ----
// where my runs of a class start (mask = my own word): a class bit after a window that does not have the class
__device__ __forceinline__ uint32_t class_starts(uint32_t mask, const uint32_t *s_mask) {
    const int t = threadIdx.x;
    const uint32_t carry = t > 0 ? (s_mask[t - 1] >> 15) & 1u : 0u;
    return mask & ~((mask << 1) | carry) & 0xFFFFu;
}
// TileRuns::ends of a tile with one class (kind 1) ...
__device__ __forceinline__ uint32_t tile_ends(const uint32_t *s_mask) { return (s_mask[0] & 1u) | (((s_mask[RP_THREADS - 1] >> 15) & 1u) << 2); }
// ... and with two classes that no window has both of
__device__ __forceinline__ uint32_t tile_ends2(const uint32_t *s_a, const uint32_t *s_b, uint32_t kind_a, uint32_t kind_b) {
    const uint32_t a0 = s_a[0], b0 = s_b[0], aL = s_a[RP_THREADS - 1], bL = s_b[RP_THREADS - 1];
    const uint32_t first = (a0 & 1u) ? kind_a : (b0 & 1u) ? kind_b : 0u;
    const uint32_t last = ((aL >> 15) & 1u) ? kind_a : ((bL >> 15) & 1u) ? kind_b : 0u;
    return first | (last << 2);
}
// The run of the class K that starts at window pos of the tile, walked to its or the tile's end: its length.  piece(g, b, pos, len) is
// called for every stretch of it inside one group: windows pos .. pos + len) = bits b .. b + len) of group g (len == RP_GROUP: the whole group).
template <class Piece> __device__ __forceinline__ uint64_t walk_run(const uint32_t *__restrict__ K, int pos, Piece &&piece) {
    uint64_t nk = 0;
    while (pos < RP_TILE) {
        const int g = pos >> 4, b = pos & 15;
        const uint32_t U = K[g] >> b;
        const int len = __builtin_ctz(~U);            // (bits 16.. of U are clear: len <= 16 - b)
        if (len == 0) break;
        piece(g, b, pos, len);
        nk += len;
        pos += len;
        if (b + len < RP_GROUP) break;
    }
    return nk;
}

// 1 if the first partial run of tile i continues the last one of tile i - 1: the same non-zero class on both sides of the seam
__device__ __forceinline__ uint32_t tile_continues(const ScanTile *__restrict__ tiles, const TileRuns *__restrict__ tout, uint64_t i) {
    if (i == 0 || tiles[i].idx == 0) return 0u;         // (idx > 0: tile i - 1 is the tile before it in the same sequence)
    const uint32_t f = ends_first(tout[i].ends);
    return f != 0u && f == ends_last(tout[i - 1].ends) ? 1u : 0u;
}

template <class Run>
__global__ __launch_bounds__(256) void scan_stitch_kernel(const ScanTile *__restrict__ tiles, const TileRuns *__restrict__ tout, const unsigned long long *__restrict__ head_base,
                                                          uint64_t ntiles, const Run *__restrict__ part, Run *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ntiles; i += nwv) {
        const TileRuns O = tout[i];
        const uint32_t cont = tile_continues(tiles, tout, i);
        for (uint32_t j = lane + cont; j < O.nruns; j += 64) {
            Run r = part[O.base + j];
            const uint32_t kind = kind_of(r);
            if (j == O.nruns - 1 && ends_last(O.ends) != 0u) {      // (the run that holds the tile's last window is its last one: `kind` is that class)
                for (uint64_t q = i + 1; q < ntiles && tiles[q].idx != 0; ++q) {
                    const TileRuns Q = tout[q];
                    if (ends_first(Q.ends) != kind) break;
                    r = absorb(r, part[Q.base]);
                    if (Q.nruns != 1 || ends_last(Q.ends) != kind) break;      // that run ends inside tile q
                }
            }
            out[head_base[i] + j - cont] = r;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct Events {                                         // a pair of HIP events around what is timed
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int create(std::string &err) {
        for (hipEvent_t &x : e) HIPCHK(hipEventCreate(&x));
        return 0;
    }
    int add_seconds(double &s, std::string &err) const {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
        s += ms * 1e-3;
        return 0;
    }
};

// Sequences in host memory as one text in workspace slot `slot` of T (16 bytes of slack after it), on T's stream.  H has to live until the
// scan's last wait has returned: it holds the one staging copy that many sequences are gathered into.  `what` starts the error messages.
struct HostText {
    uint8_t *d_text = nullptr;
    std::vector<int64_t> offs;
    std::vector<char> all;
};
int pack_host_text(Table &T, int slot, int n_seqs, const char *const *seqs, const int64_t *lens, const char *what, HostText &H, std::string &err);

// Every table of a scan zeroed if it is only logically empty, and whatever the other tables' streams still do to them ordered before T's
// stream, the one the scan runs on.  Entries of `others` may be null or T itself.  `order` has to live until the scan has been queued.
// (Hidden: it was file-local before it was shared, and the library's list of exported symbols stays what it was.)
__attribute__((visibility("hidden"))) int settle(Table &T, Table *const *others, int n, Events &order, std::string &err);

// The tiles of n_seqs sequences, in (sequence, position) order, and how many windows they hold.  per_seq, if given, gets each sequence's
// windows at per_seq[stride * i].  No tile is not an error (the caller has nothing to scan); tiles without a text are.
struct TileList {
    std::vector<ScanTile> tiles;
    uint64_t windows = 0;
    int64_t *d_offs = nullptr;                          // upload_tiles: the offsets and the tiles in workspace slots W + 1 and W + 2
    ScanTile *d_tiles = nullptr;
};
int build_tiles(int k, int n_seqs, const uint8_t *d_text, const int64_t *offsets, const char *what, uint64_t *per_seq, size_t stride, TileList &L, std::string &err);
int upload_tiles(Table &T, int W, int n_seqs, const int64_t *offsets, TileList &L, std::string &err);

int launch_heads(hipStream_t st, const ScanTile *d_tiles, const TileRuns *d_tout, uint64_t ntiles, unsigned long long *d_head, unsigned long long *d_ctl, std::string &err);

// A kernel that appends to a list of unknown length: launch(cap) sizes the list for cap entries and launches on st; the kernel adds what
// it WANTED to write to d_ctl[SC_CURSOR] and writes nothing that does not fit.  Zeroes d_zero[0 .. zero_words) (the control words are in
// there) before each launch, adds the kernel's event time to `seconds`, and leaves the control words in ctl.  If more was wanted than
// `cap`, it is repeated once with exactly that room (`retried`); more still is the error `changed`.
// A kernel that appends to TWO lists counts the second one in control word word2 and writes nothing that does not fit both; *cap2 is the
// second list's room, which launch reads where it sizes that list.  More wanted of either: repeated once with exactly that room for both.
template <class Launch>
int run_counted(hipStream_t st, unsigned long long *d_zero, size_t zero_words, const unsigned long long *d_ctl, unsigned long long cap, const std::string &changed,
                unsigned long long (&ctl)[SC_WORDS], double &seconds, int &retried, std::string &err, Launch &&launch, int word2 = 0, unsigned long long *cap2 = nullptr) {
    Events ev;
    if (ev.create(err)) return -1;
    for (int attempt = 0;; ++attempt) {
        HIPCHK(hipMemsetAsync(d_zero, 0, zero_words * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        if (launch(cap)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        if (ev.add_seconds(seconds, err)) return -1;
        if (ctl[SC_CURSOR] <= cap && (!cap2 || ctl[word2] <= *cap2)) return 0;
        if (attempt) { err = changed; return -1; }
        cap = std::max(cap, ctl[SC_CURSOR]);            // the kernel counted what it could not write: exactly this much room is needed
        if (cap2) *cap2 = std::max(*cap2, ctl[word2]);
        retried = 1;
    }
}

// The host stage of a front search on T's stream, after the caller has uploaded its sites: the control words and `per_seq` words per
// sequence after them live in workspace slot ctl_slot and are zeroed before each launch.  launch(cap, d_ctl, d_per) sizes the caller's
// record list for cap records, launches its kernel and returns the list (null: err is set); run_counted repeats it once if more were
// found.  Leaves the control words in ctl, the records in recs and the per-sequence words in per, all downloaded and waited for, and
// checks that column c of the per-sequence words adds up to control word sum_words[c] (`no_sum` if not).  `seconds` is the kernel's event
// time, both attempts if it was repeated.
template <class Rec, class Launch>
int search_stage(Table &T, int ctl_slot, int n_seqs, int per_seq, const int *sum_words, unsigned long long cap, const char *changed, const char *no_sum,
                 unsigned long long (&ctl)[SC_WORDS], std::vector<Rec> &recs, std::vector<unsigned long long> &per, double &seconds, int &retried, std::string &err,
                 Launch &&launch) {
    hipStream_t st = T.stream;
    const size_t words = SC_WORDS + (size_t)per_seq * (size_t)n_seqs;
    unsigned long long *d_ctl = (unsigned long long *)T.workspace(ctl_slot, words * sizeof(unsigned long long), err);
    if (!d_ctl) return -1;
    const Rec *d_rec = nullptr;
    if (run_counted(st, d_ctl, words, d_ctl, cap, changed, ctl, seconds, retried, err, [&](unsigned long long room) { return (d_rec = launch(room, d_ctl, d_ctl + SC_WORDS)) ? 0 : -1; }))
        return -1;
    recs.resize(ctl[SC_CURSOR]);
    per.resize(words - SC_WORDS);
    if (!recs.empty()) HIPCHK(hipMemcpyAsync(recs.data(), d_rec, recs.size() * sizeof(Rec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(per.data(), d_ctl + SC_WORDS, per.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    for (int c = 0; c < per_seq; ++c) {
        unsigned long long sum = 0;
        for (size_t i = 0; i < (size_t)n_seqs; ++i) sum += per[(size_t)per_seq * i + c];
        if (sum != ctl[sum_words[c]]) { err = no_sum; return -1; }
    }
    return 0;
}

// The nparts > 0 partial runs of a run scan made into final runs (workspace slot out_slot of T) and queued for download into `runs`; the
// caller waits for T's stream.  Adds the two kernels' event time to `seconds`.
template <class Run>
int stitch_runs(Table &T, int out_slot, const TileList &L, const TileRuns *d_tout, unsigned long long *d_head, const Run *d_part, uint64_t nparts, unsigned long long *d_ctl,
                const char *what, std::vector<Run> &runs, double &seconds, std::string &err) {
    hipStream_t st = T.stream;
    const uint64_t ntiles = L.tiles.size();
    Run *d_out = (Run *)T.workspace(out_slot, nparts * sizeof(Run), err);
    if (!d_out) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    unsigned long long ctl[SC_WORDS];
    HIPCHK(hipEventRecord(ev.e[0], st));
    if (launch_heads(st, L.d_tiles, d_tout, ntiles, d_head, d_ctl, err)) return -1;
    hipLaunchKernelGGL(scan_stitch_kernel<Run>, dim3((unsigned)std::min<uint64_t>((ntiles + 3) / 4, 256 * 16)), dim3(256), 0, st, L.d_tiles, d_tout, d_head, ntiles, d_part,
                       d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    HIPCHK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    if (ev.add_seconds(seconds, err)) return -1;
    const uint64_t nruns = ctl[SC_HEADS];
    if (nruns > nparts) { err = std::string(what) + ": more runs than partial runs"; return -1; }
    runs.resize(nruns);
    if (nruns) HIPCHK(hipMemcpyAsync(runs.data(), d_out, nruns * sizeof(Run), hipMemcpyDeviceToHost, st));
    return 0;
}

// The host stage of a run scan on T's stream and workspace slots W + 1 .. W + 7, after the caller has checked its arguments and settled
// its tables: `counts` gets `stride` words per sequence (the windows, then the kernel's ncount device counters), `runs` the final runs in
// (sequence, start) order.  launch(grid, st, L, ntiles, d_cnt, d_tout, d_part, cap, d_ctl) is the caller's one kernel launch.  `seconds`
// is the event time of the scan kernel (both attempts if it was repeated) and of the two stitch kernels.
template <class Run, class Launch>
int run_scan(Table &T, int W, const char *what, int n_seqs, const uint8_t *d_text, const int64_t *offsets, int ncount, size_t stride, std::vector<uint64_t> &counts,
             std::vector<Run> &runs, double &seconds, int &retried, std::string &err, Launch &&launch) {
    counts.assign((size_t)n_seqs * stride, 0);
    runs.clear();
    seconds = 0;
    retried = 0;
    TileList L;
    if (build_tiles(T.k, n_seqs, d_text, offsets, what, counts.data(), stride, L, err)) return -1;
    const uint64_t ntiles = L.tiles.size();
    if (ntiles == 0) return 0;
    hipStream_t st = T.stream;
    TileRuns *d_tout = (TileRuns *)T.workspace(W + 3, ntiles * sizeof(TileRuns), err);
    unsigned long long *d_head = (unsigned long long *)T.workspace(W + 4, ntiles * sizeof(unsigned long long), err);
    const size_t cnt_words = (size_t)n_seqs * ncount + SC_WORDS;
    unsigned long long *d_cnt = (unsigned long long *)T.workspace(W + 5, cnt_words * sizeof(unsigned long long), err);
    if (!d_tout || !d_head || !d_cnt || upload_tiles(T, W, n_seqs, offsets, L, err)) return -1;
    unsigned long long *d_ctl = d_cnt + (size_t)n_seqs * ncount, ctl[SC_WORDS] = {0, 0, 0, 0};
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 256 * 8);
    Run *d_part = nullptr;
    auto scan = [&](unsigned long long cap) {
        d_part = (Run *)T.workspace(W + 6, cap * sizeof(Run), err);
        if (!d_part) return -1;
        launch(grid, st, L, ntiles, d_cnt, d_tout, d_part, cap, d_ctl);
        return 0;
    };
    if (run_counted(st, d_cnt, cnt_words, d_ctl, L.windows / 64 + 65536, std::string(what) + ": the number of partial runs changed between two scans", ctl, seconds, retried,
                    err, scan))
        return -1;
    const uint64_t nparts = ctl[SC_CURSOR];
    std::vector<unsigned long long> cnt((size_t)n_seqs * ncount);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (nparts && stitch_runs(T, W + 7, L, d_tout, d_head, d_part, nparts, d_ctl, what, runs, seconds, err)) return -1;
    HIPCHK(jk_stream_wait(st));
    for (int i = 0; i < n_seqs; ++i)
        for (int c = 0; c < ncount; ++c) counts[stride * (size_t)i + 1 + c] = cnt[(size_t)ncount * i + c];
    return 0;
}

}  // namespace jk
