// deflate_gpu.hip -- text in HBM -> BGZF members, one workgroup per block of DF_BLOCK text bytes (semantics: include/jasper_hip.h,
// jasper_deflate_bgzf; the host arithmetic: deflate_plan.hpp).
//
//   df_member_kernel  one workgroup per block, the block's bytes in LDS.  In this order:
//                       - the literal histogram and the block's CRC-32 (a piece per thread, the pieces combined as zlib's crc32_combine
//                         combines them: a piece's CRC times x^(8 * bytes behind it), all of them XORed);
//                       - the literal-only code: length-limited Huffman lengths for the 286 literal/length symbols, a two-symbol
//                         distance code, the code-length code over the 316 lengths, and what the block costs in bits that way;
//                       - LZ77 by tiles of DF_THREADS positions: every thread takes one position, looks up the hash head of its three
//                         bytes (filled by EARLIER tiles only) and the byte before it (distance 1), measures both matches in LDS and
//                         keeps the longer if it is worth more than its literals under the literal-only code; after a barrier the tile's
//                         positions enter the hash heads with an LDS atomicMax (the highest position wins whatever order the lanes come
//                         in) and thread 0 walks the greedy parse across the tile; after another the tokens the walk has marked are
//                         counted and the matches leave for the block's record words in HBM;
//                         (a source in the SAME tile is invisible unless it is the byte before: at a position o bytes into its tile no
//                         match at a distance of 2 .. o is found, and of several earlier sources with one hash only the last is tried;
//                         DESIGN.md 4.15.3 says what that costs)
//                       - the LZ codes and their cost; the cheapest of stored / literal-only / LZ in BYTES is written: header, blocks,
//                         CRC-32 and ISIZE into the block's slot, its size into sizes[].  Token bits: a bit count per thread over its
//                         span of positions, a two-level scan over the threads, then every thread ORs its tokens into the slot's words (the first
//                         and the last word of a thread's run are shared with its neighbours and go through atomicOr, the ones between
//                         are plain stores); the slots are zero before the kernel runs.
//   rt_scan_words     (readtext.hip) the exclusive scan of the member sizes
//   df_pack_kernel    one workgroup per member: slot -> its place in the output
// Nothing here depends on the order in which lanes or workgroups run: the same text gives the same bytes.
#include "deflate_gpu.hpp"
#include "readtext.hpp"
#include "scan_tile.hpp"

namespace jk {

namespace {

#ifndef JK_DF_THREADS
#define JK_DF_THREADS 1024        // threads of a workgroup = positions of a tile (experiment builds: EXTRA=-DJK_DF_THREADS=256)
#endif
constexpr int DF_THREADS = JK_DF_THREADS;
constexpr int DF_HASH_BITS = 13;
constexpr int DF_NLL = 286, DF_ND = 30, DF_NCL = 19;
constexpr int DF_MIN_MATCH = 3, DF_MAX_MATCH = 258, DF_MAX_DIST = 32768;
constexpr int DF_SURE = 24;                     // a match this long is taken without weighing it against its literals
constexpr uint32_t DF_START = 0x8000u;          // in a tile word: the greedy parse begins a token here
enum { DFC_BLOCKS = 0, DFC_STORED = 1, DFC_LIT = 2, DFC_LZ = 3, DFC_MATCHES = 4, DFC_MATCHED = 5 };
enum { MODE_STORED = 0, MODE_LIT = 1, MODE_LZ = 2 };
enum { ACC_CRC = 0, ACC_TOK_B, ACC_HDR_B, ACC_TOK_A, ACC_HDR_A, ACC_EXTRA, ACC_MATCHES, ACC_MATCHED, ACC_WORDS };
constexpr int DF_TILES = (DF_BLOCK + DF_THREADS - 1) / DF_THREADS;
static_assert(DF_THREADS >= 256 && DF_THREADS % 64 == 0, "the CRC table is filled by the first 256 threads, the bitmaps one 64-bit ballot per wave");

// ---- CRC-32 combination (GF(2) polynomial arithmetic, as zlib's crc32_combine and the inflater's host code have it) ----
constexpr uint32_t df_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
struct X2N { uint32_t t[32]; };
constexpr X2N df_make_x2n() {
    X2N x{};
    uint32_t p = 1u << 30;
    x.t[0] = p;
    for (int i = 1; i < 32; ++i) x.t[i] = p = df_multmodp(p, p);
    return x;
}
__constant__ X2N df_x2n = df_make_x2n();
__device__ uint32_t df_x2nmodp(uint32_t n, unsigned k) {      // x^(n * 2^k) modulo p(x)
    uint32_t p = 1u << 31;
    while (n) {
        if (n & 1) p = df_multmodp(df_x2n.t[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

// ---- the deflate alphabet ----
__device__ __forceinline__ uint32_t len_extra_bits(uint32_t len) {
    const uint32_t l = len - 3;
    return (l < 8 || len == 258) ? 0 : (31 - __clz(l)) - 2;
}
__device__ __forceinline__ uint32_t len_symbol(uint32_t len, uint32_t &extra, uint32_t &eb) {
    const uint32_t l = len - 3;
    extra = 0;
    eb = 0;
    if (len == 258) return 285;
    if (l < 8) return 257 + l;
    eb = (31 - __clz(l)) - 2;
    extra = l & ((1u << eb) - 1);
    return 257 + 4 * eb + 4 + ((l >> eb) & 3);
}
__device__ __forceinline__ uint32_t dist_extra_bits(uint32_t dist) {
    const uint32_t d = dist - 1;
    return d < 4 ? 0 : (31 - __clz(d)) - 1;
}
__device__ __forceinline__ uint32_t dist_symbol(uint32_t dist, uint32_t &extra, uint32_t &eb) {
    const uint32_t d = dist - 1;
    extra = 0;
    eb = 0;
    if (d < 4) return d;
    const uint32_t k = 31 - __clz(d);
    eb = k - 1;
    extra = d & ((1u << eb) - 1);
    return 2 * k + ((d >> (k - 1)) & 1);
}

// the four text bytes from byte i on (any i; the text has 16 bytes of room behind it): two aligned words and a byte shift
__device__ __forceinline__ uint32_t text4(const uint32_t *text, uint32_t i) {
    return __builtin_amdgcn_alignbyte(text[(i >> 2) + 1], text[i >> 2], i & 3);
}
// how many bytes from a on equal those from b on, `most` at the most: four at a time, the first unequal byte by its place in the XOR
__device__ __forceinline__ uint32_t match_length(const uint32_t *text, uint32_t a, uint32_t b, uint32_t most) {
    uint32_t l = 0;
    while (l < most) {
        const uint32_t x = text4(text, a + l) ^ text4(text, b + l);
        if (x) {
            l += (uint32_t)(__ffs(x) - 1) >> 3;
            break;
        }
        l += 4;
    }
    return l < most ? l : most;
}

// ---- LDS ----
struct HuffScratch {
    uint32_t w[288];        // the weights the code is built from: the frequencies, halved (never to 0) while the code is too deep
    uint32_t lw[288];       // the leaves' weights in ascending order
    uint32_t iw[288];       // the inner nodes' weights in the order they are made (ascending too)
    uint16_t sym[288];      // sorted leaf -> symbol
    uint16_t lpar[288];     // sorted leaf -> the inner node above it
    uint16_t ipar[288];     // inner node -> the inner node above it
    uint16_t idep[288];     // inner node -> its depth
    uint32_t nz, maxlen;
    uint32_t blc[16], next[16];
};
struct DeflateLds {
    uint32_t text[(DF_BLOCK + 16) / 4];
    union {
        uint32_t head[1 << DF_HASH_BITS];       // hash of three bytes -> the last position + 1 that had it, 0: none (during the tiles)
        HuffScratch hs;                         // (before and after them)
    } u;
    uint32_t starts[DF_TILES * DF_THREADS / 32];    // a bit per position: a token of the greedy parse begins here
    uint32_t matches[DF_TILES * DF_THREADS / 32];   // ... and it is a match
    uint32_t tile[DF_THREADS];
    uint32_t hist_lit[288], hist_ll[288], hist_d[32], hist_cl[20];
    uint32_t crc_tab[256];
    uint32_t sums[DF_THREADS], group_sums[DF_THREADS / 32];
    uint32_t acc[ACC_WORDS];
    uint16_t ll_code[288], d_code[32], cl_code[20];
    uint8_t llA[288], llB[288], dA[32], dB[32], clA[20], clB[20];
};
static_assert(sizeof(DeflateLds) <= 160 * 1024, "one workgroup's LDS");

// Huffman code lengths of at most `limit` bits for freq[0 .. nsym), by the whole workgroup.  A code has at least two symbols (symbols of
// frequency 0 are drafted, lowest first), so it is always complete.  Symbols sorted by (weight, symbol) with a rank per thread, then one
// thread merges leaves and inner nodes from two queues.  A code deeper than the limit is built again from halved weights (1 stays 1):
// equal weights end in a code of depth ceil(log2(symbols)), 9 for the 286 and 5 for the 19, so the loop ends.
__device__ void huff_lengths(const uint32_t *freq, int nsym, uint32_t limit, uint8_t *len, HuffScratch &S) {
    const int t = threadIdx.x;
    for (int i = t; i < nsym; i += DF_THREADS) S.w[i] = freq[i];
    if (t == 0) S.nz = 0;
    __syncthreads();
    for (int i = t; i < nsym; i += DF_THREADS)
        if (S.w[i]) atomicAdd(&S.nz, 1u);
    __syncthreads();
    if (t == 0 && S.nz < 2) {
        uint32_t nz = S.nz;
        for (int i = 0; i < nsym && nz < 2; ++i)
            if (!S.w[i]) { S.w[i] = 1; ++nz; }
        S.nz = nz;
    }
    __syncthreads();
    const int m = (int)S.nz;
    for (;;) {
        if (t == 0) S.maxlen = 0;
        for (int i = t; i < nsym; i += DF_THREADS) {
            const uint32_t w = S.w[i];
            if (!w) continue;
            int r = 0;
            for (int j = 0; j < nsym; ++j) {
                const uint32_t wj = S.w[j];
                r += (wj != 0 && (wj < w || (wj == w && j < i))) ? 1 : 0;
            }
            S.sym[r] = (uint16_t)i;
            S.lw[r] = w;
        }
        __syncthreads();
        if (t == 0) {
            int li = 0, ii = 0;
            for (int k = 0; k < m - 1; ++k) {
                uint32_t s = 0;
                for (int q = 0; q < 2; ++q) {
                    const bool leaf = li < m && (ii >= k || S.lw[li] <= S.iw[ii]);
                    if (leaf) { s += S.lw[li]; S.lpar[li] = (uint16_t)k; ++li; }
                    else { s += S.iw[ii]; S.ipar[ii] = (uint16_t)k; ++ii; }
                }
                S.iw[k] = s;
            }
            S.idep[m - 2] = 0;
            for (int k = m - 3; k >= 0; --k) S.idep[k] = (uint16_t)(S.idep[S.ipar[k]] + 1);
        }
        __syncthreads();
        for (int r = t; r < m; r += DF_THREADS) {
            const uint32_t d = (uint32_t)S.idep[S.lpar[r]] + 1;
            len[S.sym[r]] = (uint8_t)d;
            atomicMax(&S.maxlen, d);
        }
        __syncthreads();
        const uint32_t deepest = S.maxlen;
        if (deepest <= limit) break;
        __syncthreads();                                // (everyone has read maxlen before it is reset)
        for (int i = t; i < nsym; i += DF_THREADS)
            if (S.w[i]) S.w[i] = (S.w[i] + 1) >> 1;
        __syncthreads();
    }
    for (int i = t; i < nsym; i += DF_THREADS)
        if (!S.w[i]) len[i] = 0;
    __syncthreads();
}

// canonical codes of the lengths, bit-reversed: what goes into an LSB-first stream
__device__ void huff_codes(const uint8_t *len, int nsym, uint16_t *code, HuffScratch &S) {
    const int t = threadIdx.x;
    if (t < 16) S.blc[t] = 0;
    __syncthreads();
    for (int i = t; i < nsym; i += DF_THREADS)
        if (len[i]) atomicAdd(&S.blc[len[i]], 1u);
    __syncthreads();
    if (t == 0) {
        uint32_t c = 0;
        S.blc[0] = 0;
        for (int b = 1; b < 16; ++b) {
            c = (c + S.blc[b - 1]) << 1;
            S.next[b] = c;
        }
    }
    __syncthreads();
    for (int i = t; i < nsym; i += DF_THREADS) {
        const uint32_t l = len[i];
        uint32_t c = 0;
        if (l) {
            uint32_t r = 0;
            for (int j = 0; j < i; ++j) r += len[j] == l ? 1 : 0;
            c = __brev(S.next[l] + r) >> (32 - l);
        }
        code[i] = (uint16_t)c;
    }
    __syncthreads();
}

// the code-length code's histogram over the 316 lengths a header sends, one by one (no run-length symbols)
__device__ void cl_histogram(const uint8_t *ll, const uint8_t *d, uint32_t *hist) {
    const int t = threadIdx.x;
    if (t < 20) hist[t] = 0;
    __syncthreads();
    for (int i = t; i < DF_NLL; i += DF_THREADS) atomicAdd(&hist[ll[i]], 1u);
    if (t < DF_ND) atomicAdd(&hist[d[t]], 1u);
    __syncthreads();
}

// sum of freq[i] * len[i] into *acc (zero before)
__device__ void add_cost(const uint32_t *freq, const uint8_t *len, int nsym, uint32_t *acc) {
    uint32_t s = 0;
    for (int i = threadIdx.x; i < nsym; i += DF_THREADS) s += freq[i] * len[i];
    if (s) atomicAdd(acc, s);
}

// bits ORed into a zeroed stream of words, any thread, any place
__device__ __forceinline__ void put_bits(uint32_t *w, uint32_t bitpos, uint32_t val, uint32_t nb) {
    if (!nb) return;
    const uint64_t v = (uint64_t)val << (bitpos & 31);
    if ((uint32_t)v) atomicOr(&w[bitpos >> 5], (uint32_t)v);
    if (v >> 32) atomicOr(&w[(bitpos >> 5) + 1], (uint32_t)(v >> 32));
}

__constant__ uint8_t df_cl_order[DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__constant__ uint8_t df_head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0};      // a member's header before BSIZE
constexpr uint32_t DF_DYN_FIXED_BITS = 3 + 5 + 5 + 4 + 3 * DF_NCL;      // BFINAL, BTYPE, HLIT, HDIST, HCLEN, the 19 code-length lengths

__global__ __launch_bounds__(DF_THREADS) void df_member_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ aux, uint8_t *__restrict__ slots,
                                                               uint64_t *__restrict__ sizes, unsigned long long *__restrict__ ctl) {
    __shared__ DeflateLds L;
    const uint32_t t = threadIdx.x;
    const uint64_t blk = blockIdx.x;
    const uint64_t base = blk * DF_BLOCK;
    const uint32_t bn = (uint32_t)(n - base < (uint64_t)DF_BLOCK ? n - base : (uint64_t)DF_BLOCK);
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(L.text);
    uint32_t *maux = aux + blk * DF_AUX_WORDS;
    uint8_t *slot = slots + blk * DF_SLOT;
    uint32_t *slotw = reinterpret_cast<uint32_t *>(slot);

    // ---- the text, the CRC table, the literal histogram, the CRC
    for (uint32_t o = t * 16; o < DF_BLOCK + 16; o += DF_THREADS * 16) {
        const Raw16 r = load16(text + base, (int64_t)o, (int64_t)bn);
        L.text[o / 4] = r.w[0]; L.text[o / 4 + 1] = r.w[1]; L.text[o / 4 + 2] = r.w[2]; L.text[o / 4 + 3] = r.w[3];
    }
    if (t < 256) {
        uint32_t c = t;
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        L.crc_tab[t] = c;
    }
    for (uint32_t i = t; i < 288; i += DF_THREADS) L.hist_lit[i] = L.hist_ll[i] = 0;
    if (t < 32) L.hist_d[t] = 0;
    if (t < ACC_WORDS) L.acc[t] = 0;
    __syncthreads();
    for (uint32_t wi = t; wi * 4 < bn; wi += DF_THREADS) {
        uint32_t w = L.text[wi];
        for (uint32_t q = 0; q < 4 && wi * 4 + q < bn; ++q) { atomicAdd(&L.hist_lit[w & 0xFF], 1u); w >>= 8; }
    }
    const uint32_t span = (bn + DF_THREADS - 1) / DF_THREADS;       // positions per thread, wherever threads take a run of them
    const uint32_t s0 = t * span < bn ? t * span : bn, s1 = s0 + span < bn ? s0 + span : bn;
    if (s1 > s0) {
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t p = s0; p < s1; ++p) c = L.crc_tab[(c ^ tb[p]) & 0xFF] ^ (c >> 8);
        atomicXor(&L.acc[ACC_CRC], df_multmodp(df_x2nmodp(bn - s1, 3), ~c));
    }
    if (t == 0) L.hist_lit[256] = 1;                                // (no literal is symbol 256: thread 0 alone writes it)
    __syncthreads();

    // ---- literals only: the code and its cost
    huff_lengths(L.hist_lit, DF_NLL, 15, L.llB, L.u.hs);
    if (t < 32) L.dB[t] = t < 2 ? 1 : 0;
    __syncthreads();
    cl_histogram(L.llB, L.dB, L.hist_cl);
    huff_lengths(L.hist_cl, DF_NCL, 7, L.clB, L.u.hs);
    add_cost(L.hist_cl, L.clB, DF_NCL, &L.acc[ACC_HDR_B]);
    add_cost(L.hist_lit, L.llB, DF_NLL, &L.acc[ACC_TOK_B]);
    __syncthreads();

    // ---- LZ77 by tiles
    for (uint32_t i = t; i < (1u << DF_HASH_BITS); i += DF_THREADS) L.u.head[i] = 0;
    __syncthreads();
    const uint32_t ntiles = (bn + DF_THREADS - 1) / DF_THREADS;
    uint32_t walk = 0;                                              // thread 0: where the greedy parse's next token begins
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        const uint32_t p = tile * DF_THREADS + t;
        const bool hashed = p + 2 < bn;
        uint32_t h = 0, m = 0;
        if (hashed) {
            h = (((uint32_t)tb[p] | ((uint32_t)tb[p + 1] << 8) | ((uint32_t)tb[p + 2] << 16)) * 0x9E3779B1u) >> (32 - DF_HASH_BITS);
            const uint32_t most = bn - p < (uint32_t)DF_MAX_MATCH ? bn - p : (uint32_t)DF_MAX_MATCH;
            uint32_t best = 0, dist = 0;
            const uint32_t hv = L.u.head[h];
            if (hv && p - (hv - 1) <= (uint32_t)DF_MAX_DIST) {      // (the LDS holds more history than a distance can name)
                best = match_length(L.text, hv - 1, p, most);
                dist = p - (hv - 1);
            }
            if (p >= 1 && dist != 1) {                              // the byte before: runs, which the heads of earlier tiles cannot give
                const uint32_t l = match_length(L.text, p - 1, p, most);
                if (l >= best) { best = l; dist = 1; }
            }
            if (best >= (uint32_t)DF_MIN_MATCH) {
                bool take = best >= (uint32_t)DF_SURE;
                if (!take) {                                        // is it cheaper than its bytes as literals?  (8 and 5: typical code lengths)
                    uint32_t lit = 0;
                    for (uint32_t l = 0; l < best; ++l) lit += L.llB[tb[p + l]];
                    take = lit > 8 + len_extra_bits(best) + 5 + dist_extra_bits(dist);
                }
                if (take) m = best | ((dist - 1) << 16);
            }
        }
        L.tile[t] = m;
        __syncthreads();
        if (hashed) atomicMax(&L.u.head[h], p + 1);
        if (t == 0) {
            const uint32_t first = tile * DF_THREADS, end = first + DF_THREADS < bn ? first + DF_THREADS : bn;
            while (walk < end) {
                const uint32_t mm = L.tile[walk - first];
                L.tile[walk - first] = mm | DF_START;
                const uint32_t l = mm & 0x1FFu;
                walk += l ? l : 1;
            }
        }
        __syncthreads();
        const uint32_t mm = L.tile[t];
        const bool start = (mm & DF_START) != 0;
        const uint32_t len = mm & 0x1FFu;
        if (start && len) {
            const uint32_t dist = (mm >> 16) + 1;
            uint32_t ex, eb, dex, deb;
            atomicAdd(&L.hist_ll[len_symbol(len, ex, eb)], 1u);
            atomicAdd(&L.hist_d[dist_symbol(dist, dex, deb)], 1u);
            atomicAdd(&L.acc[ACC_EXTRA], eb + deb);
            atomicAdd(&L.acc[ACC_MATCHES], 1u);
            atomicAdd(&L.acc[ACC_MATCHED], len);
            maux[p / 3] = mm & ~DF_START;
        } else if (start) {
            atomicAdd(&L.hist_ll[tb[p]], 1u);
        }
        const unsigned long long sb = __ballot(start), mb = __ballot(start && len);
        if ((t & 63) == 0) {
            const uint32_t wi = tile * (DF_THREADS / 32) + (t >> 6) * 2;
            L.starts[wi] = (uint32_t)sb; L.starts[wi + 1] = (uint32_t)(sb >> 32);
            L.matches[wi] = (uint32_t)mb; L.matches[wi + 1] = (uint32_t)(mb >> 32);
        }
    }
    if (t == 0) L.hist_ll[256] = 1;
    __syncthreads();

    // ---- LZ: the codes and their cost
    huff_lengths(L.hist_ll, DF_NLL, 15, L.llA, L.u.hs);
    huff_lengths(L.hist_d, DF_ND, 15, L.dA, L.u.hs);
    cl_histogram(L.llA, L.dA, L.hist_cl);
    huff_lengths(L.hist_cl, DF_NCL, 7, L.clA, L.u.hs);
    add_cost(L.hist_cl, L.clA, DF_NCL, &L.acc[ACC_HDR_A]);
    add_cost(L.hist_ll, L.llA, DF_NLL, &L.acc[ACC_TOK_A]);
    add_cost(L.hist_d, L.dA, DF_ND, &L.acc[ACC_TOK_A]);
    __syncthreads();

    // ---- the cheapest in bytes (a tie goes to the simpler one)
    const uint32_t hdrA = DF_DYN_FIXED_BITS + L.acc[ACC_HDR_A], hdrB = DF_DYN_FIXED_BITS + L.acc[ACC_HDR_B];
    const uint32_t bytesA = (hdrA + L.acc[ACC_TOK_A] + L.acc[ACC_EXTRA] + 7) / 8, bytesB = (hdrB + L.acc[ACC_TOK_B] + 7) / 8;
    uint32_t mode = MODE_STORED, payload = bn + DF_STORED;
    if (bytesB < payload) { mode = MODE_LIT; payload = bytesB; }
    if (bytesA < payload) { mode = MODE_LZ; payload = bytesA; }
    const uint32_t member = DF_HEAD + payload + DF_TAIL;
    const uint32_t crc = L.acc[ACC_CRC];
    auto head = [&](int i) -> uint32_t { return i < 16 ? df_head[i] : i == 16 ? ((member - 1) & 0xFF) : ((member - 1) >> 8); };
    if (t == 0) {
        sizes[blk] = member;
        atomicAdd(&ctl[DFC_BLOCKS], 1ull);
        atomicAdd(&ctl[mode == MODE_STORED ? DFC_STORED : mode == MODE_LIT ? DFC_LIT : DFC_LZ], 1ull);
        if (mode == MODE_LZ) {
            atomicAdd(&ctl[DFC_MATCHES], (unsigned long long)L.acc[ACC_MATCHES]);
            atomicAdd(&ctl[DFC_MATCHED], (unsigned long long)L.acc[ACC_MATCHED]);
        }
    }

    if (mode == MODE_STORED) {                                      // bytes, each stored once
        if (t == 0) {
            for (int i = 0; i < DF_HEAD; ++i) slot[i] = (uint8_t)head(i);
            slot[DF_HEAD] = 1;
            slot[DF_HEAD + 1] = (uint8_t)(bn & 0xFF); slot[DF_HEAD + 2] = (uint8_t)(bn >> 8);
            slot[DF_HEAD + 3] = (uint8_t)(~bn & 0xFF); slot[DF_HEAD + 4] = (uint8_t)((~bn >> 8) & 0xFF);
            uint8_t *tail = slot + DF_HEAD + DF_STORED + bn;
            for (int i = 0; i < 4; ++i) { tail[i] = (uint8_t)(crc >> (8 * i)); tail[4 + i] = (uint8_t)(bn >> (8 * i)); }
        }
        for (uint32_t p = t; p < bn; p += DF_THREADS) slot[DF_HEAD + DF_STORED + p] = tb[p];
        return;
    }

    // ---- a dynamic block: the codes, the header (thread 0), the tokens (everyone)
    const uint8_t *ll = mode == MODE_LZ ? L.llA : L.llB, *dl = mode == MODE_LZ ? L.dA : L.dB, *cl = mode == MODE_LZ ? L.clA : L.clB;
    const uint32_t hdr = mode == MODE_LZ ? hdrA : hdrB;
    huff_codes(ll, DF_NLL, L.ll_code, L.u.hs);
    huff_codes(dl, DF_ND, L.d_code, L.u.hs);
    huff_codes(cl, DF_NCL, L.cl_code, L.u.hs);
    const bool lz = mode == MODE_LZ;
    uint32_t mine = 0;
    for (uint32_t p = s0; p < s1; ++p) {
        if (lz && !((L.starts[p >> 5] >> (p & 31)) & 1)) continue;
        if (lz && ((L.matches[p >> 5] >> (p & 31)) & 1)) {
            const uint32_t mm = maux[p / 3];
            uint32_t ex, eb, dex, deb;
            mine += ll[len_symbol(mm & 0x1FFu, ex, eb)] + eb;
            mine += dl[dist_symbol((mm >> 16) + 1, dex, deb)] + deb;
        } else {
            mine += ll[tb[p]];
        }
    }
    // the scan over the threads in two levels: within a group of 32 threads by reading the group's sums, then over the groups' totals
    L.sums[t] = mine;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t j = t & ~31u; j < t; ++j) before += L.sums[j];
    if ((t & 31) == 31) L.group_sums[t >> 5] = before + mine;
    __syncthreads();
    uint32_t bp = DF_HEAD * 8 + hdr + before, all = 0;
    for (uint32_t g = 0; g < DF_THREADS / 32; ++g) {
        const uint32_t s = L.group_sums[g];
        if (g < (t >> 5)) bp += s;
        all += s;
    }
    if (t == 0) {
        uint32_t at = 0;
        for (int i = 0; i < DF_HEAD; ++i, at += 8) put_bits(slotw, at, head(i), 8);
        put_bits(slotw, at, 1u | (2u << 1), 3); at += 3;           // BFINAL = 1, BTYPE = 2
        put_bits(slotw, at, DF_NLL - 257, 5); at += 5;
        put_bits(slotw, at, DF_ND - 1, 5); at += 5;
        put_bits(slotw, at, DF_NCL - 4, 4); at += 4;
        for (int i = 0; i < DF_NCL; ++i, at += 3) put_bits(slotw, at, cl[df_cl_order[i]], 3);
        for (int i = 0; i < DF_NLL; ++i) { const uint32_t s = ll[i]; put_bits(slotw, at, L.cl_code[s], cl[s]); at += cl[s]; }
        for (int i = 0; i < DF_ND; ++i) { const uint32_t s = dl[i]; put_bits(slotw, at, L.cl_code[s], cl[s]); at += cl[s]; }
        put_bits(slotw, DF_HEAD * 8 + hdr + all, L.ll_code[256], ll[256]);      // the end of the block behind the last token
        const uint32_t tail = (DF_HEAD + payload) * 8;
        put_bits(slotw, tail, crc, 32);
        put_bits(slotw, tail + 32, bn, 32);
    }
    uint32_t wi = bp >> 5, ab = bp & 31;
    uint64_t acc = 0;
    bool first = true;
    auto push = [&](uint32_t v, uint32_t nb) {
        acc |= (uint64_t)v << ab;
        ab += nb;
        while (ab >= 32) {
            if (first) { atomicOr(&slotw[wi], (uint32_t)acc); first = false; }
            else slotw[wi] = (uint32_t)acc;
            ++wi;
            acc >>= 32;
            ab -= 32;
        }
    };
    for (uint32_t p = s0; p < s1; ++p) {
        if (lz && !((L.starts[p >> 5] >> (p & 31)) & 1)) continue;
        if (lz && ((L.matches[p >> 5] >> (p & 31)) & 1)) {
            const uint32_t mm = maux[p / 3];
            uint32_t ex, eb, dex, deb;
            const uint32_t ls = len_symbol(mm & 0x1FFu, ex, eb), ds = dist_symbol((mm >> 16) + 1, dex, deb);
            push((uint32_t)L.ll_code[ls] | (ex << ll[ls]), ll[ls] + eb);
            push((uint32_t)L.d_code[ds] | (dex << dl[ds]), dl[ds] + deb);
        } else {
            const uint32_t b = tb[p];
            push(L.ll_code[b], ll[b]);
        }
    }
    if (ab && (uint32_t)acc) atomicOr(&slotw[wi], (uint32_t)acc);
}

__global__ __launch_bounds__(DF_THREADS) void df_pack_kernel(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ pre, uint8_t *__restrict__ out) {
    const uint64_t blk = blockIdx.x;
    const uint64_t off = pre[blk];
    const uint32_t size = (uint32_t)(pre[blk + 1] - off);
    const uint8_t *src = slots + blk * DF_SLOT;
    struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
    for (uint32_t o = threadIdx.x * 16; o < size; o += DF_THREADS * 16) {
        if (o + 16 <= size) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + o);      // (a slot begins at a multiple of 64 KiB)
            V16 u;
            u.w[0] = v.x; u.w[1] = v.y; u.w[2] = v.z; u.w[3] = v.w;
            *reinterpret_cast<V16 *>(out + off + o) = u;
        } else {
            for (uint32_t j = o; j < size; ++j) out[off + j] = src[j];
        }
    }
}

const char *const DF_WHAT = "deflate";

}  // namespace

int deflate_device(Table &T, const uint8_t *d_text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_bytes, uint64_t *counters, double *seconds, std::string &err) {
    const std::string w(DF_WHAT);
    if (!out_bytes || out_cap < 0) { err = w + ": bad arguments"; return -1; }
    *out_bytes = 0;
    if (deflate_check(n) != DF_OK) { err = w + ": more than 2^31-1 text bytes in one call"; return -1; }
    if (n == 0) return 0;
    if (!d_text || !out) { err = w + ": bad arguments"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    hipStream_t st = T.stream;
    const uint64_t un = (uint64_t)n, nb = deflate_blocks(un);
    const DeflateBuffers B = deflate_buffers(un, RT_BLOCK);
    const int W = Table::WS_DEFLATE;
    uint8_t *d_slots = (uint8_t *)T.workspace(W + 1, B.slots, err);
    uint32_t *d_aux = (uint32_t *)T.workspace(W + 2, B.aux, err);
    uint64_t *d_sizes = (uint64_t *)T.workspace(W + 3, B.sizes, err);
    uint64_t *d_pre = (uint64_t *)T.workspace(W + 4, B.pre, err);
    uint64_t *d_blk = (uint64_t *)T.workspace(W + 5, B.scan_blocks, err);
    uint8_t *d_out = (uint8_t *)T.workspace(W + 6, B.out, err);
    unsigned long long *d_ctl = (unsigned long long *)T.workspace(W + 7, DF_COUNTERS * sizeof(unsigned long long), err);
    if (!d_slots || !d_aux || !d_sizes || !d_pre || !d_blk || !d_out || !d_ctl) return -1;
    HIPCHK(hipMemsetAsync(d_ctl, 0, DF_COUNTERS * sizeof(unsigned long long), st));
    Events ev;
    if (ev.create(err)) return -1;
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(hipMemsetAsync(d_slots, 0, (size_t)nb * DF_SLOT, st));
    hipLaunchKernelGGL(df_member_kernel, dim3((unsigned)nb), dim3(DF_THREADS), 0, st, d_text, un, d_aux, d_slots, d_sizes, d_ctl);
    HIPCHK(hipGetLastError());
    if (rt_scan_words(st, d_sizes, nb, d_blk, d_pre, err)) return -1;
    hipLaunchKernelGGL(df_pack_kernel, dim3((unsigned)nb), dim3(DF_THREADS), 0, st, d_slots, d_pre, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    uint64_t total = 0;
    unsigned long long c[DF_COUNTERS] = {0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(&total, d_pre + nb, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c, d_ctl, sizeof c, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) *seconds += s;
    if (total > deflate_bound(un) || c[DFC_BLOCKS] != nb) { err = w + ": the kernels left members that pass their bound"; return -1; }
    if (total > (uint64_t)out_cap) { err = w + ": the members do not fit the output buffer (jasper_deflate_bound says how large it must be)"; return -1; }
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    if (counters)
        for (int i = 0; i < DF_COUNTERS; ++i) counters[i] += c[i];
    *out_bytes = (int64_t)total;
    return 0;
}

int deflate_host(Table &T, const uint8_t *text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_bytes, uint64_t *counters, double *seconds, std::string &err) {
    const std::string w(DF_WHAT);
    if (counters)
        for (int i = 0; i < DF_COUNTERS; ++i) counters[i] = 0;
    if (seconds) *seconds = 0;
    if (out_bytes) *out_bytes = 0;
    if (deflate_check(n) != DF_OK) { err = w + ": more than 2^31-1 text bytes in one call"; return -1; }
    uint8_t *d_text = nullptr;
    if (n > 0) {
        if (!text) { err = w + ": null text"; return -1; }
        HIPCHK(hipSetDevice(T.device));
        uint8_t *room = (uint8_t *)T.workspace(Table::WS_DEFLATE, deflate_buffers((uint64_t)n, RT_BLOCK).text, err);
        if (!room) return -1;
        d_text = room + ((uintptr_t)text & 15u);        // (the kernel takes any alignment; the tests reach every one through the host pointer)
        HIPCHK(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, T.stream));
    }
    return deflate_device(T, d_text, n, out, out_cap, out_bytes, counters, seconds, err);
}

}  // namespace jk
