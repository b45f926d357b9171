// inflate_gpu.hip -- one gzip stream inflated on the GPU (stages and rules: inflate_gpu.hpp).
#include "inflate_gpu.hpp"
#include <zlib.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace jk {

namespace {

constexpr uint32_t GZ_WIN = 32768;
constexpr int GZ_MAXM = 32;            // member ends one decoder records; one more ends the decoder at that boundary (a gap)
constexpr int LIT_BITS = 10, DIST_BITS = 8;
constexpr size_t GZ_PIECE = 16u << 10;  // CRC piece (bytes)
constexpr size_t GZ_MARGIN = 4u << 20;  // compressed bytes past a slab's nominal end: its last block ends in there
constexpr uint64_t NONE = ~0ull;
enum { GZ_STOP = 0, GZ_SLAB_END = 1, GZ_EOF = 2, GZ_GAP = 3, GZ_ERR = 4 };

// what one decoder reports
struct GzdRec {
    unsigned long long end_bit;        // STOP / SLAB_END: the boundary it stopped at; GAP: the last block start it reached
    unsigned long long out_len;        // symbols up to end_bit
    unsigned int status, n_members;    // member ends before end_bit
    unsigned long long m_off[GZ_MAXM]; // output offset of each member end, its trailer
    unsigned int m_crc[GZ_MAXM], m_isize[GZ_MAXM];
};

// ---- device helpers ----------------------------------------------------------------------------------------------------

// RFC 1952 member header at byte o: its length, 0 if there is none, -1 if the buffer ends first (the rules of
// ParallelGunzip::gzip_header_len with n = the file's length when the buffer reaches the end of the file)
__device__ __host__ inline long gz_header_len(const uint8_t *p, uint64_t n, uint64_t o, bool at_end) {
    const long shortv = at_end ? 0 : -1;
    if (o + 18 > n) return shortv;
    if (p[o] != 0x1f || p[o + 1] != 0x8b || p[o + 2] != 8 || (p[o + 3] & 0xE0)) return 0;
    const int flg = p[o + 3];
    uint64_t q = o + 10;
    if (flg & 4) { if (q + 2 > n) return shortv; const uint64_t xlen = p[q] | (p[q + 1] << 8); q += 2 + xlen; }
    if (flg & 8) { while (q < n && p[q]) ++q; ++q; }
    if (flg & 16) { while (q < n && p[q]) ++q; ++q; }
    if (flg & 2) q += 2;
    return q < n ? (long)(q - o) : shortv;
}

struct SlowBits {
    const uint8_t *d; uint64_t n, pos; bool ok;
    __device__ uint32_t get(int k) {
        uint32_t v = 0;
        for (int i = 0; i < k; ++i) {
            const uint64_t by = pos >> 3;
            if (by >= n) { ok = false; return 0; }
            v |= (uint32_t)((d[by] >> (pos & 7)) & 1u) << i;
            ++pos;
        }
        return v;
    }
};

__device__ bool dg_complete(const int *count, int n_nonzero, int maxbits, bool allow_single, int n) {
    if (n_nonzero == 0) return allow_single;
    int left = 1;
    for (int l = 1; l <= maxbits; ++l) { left <<= 1; left -= count[l]; if (left < 0) return false; }
    if (left == 0) return true;
    return allow_single && n_nonzero == 1 && count[1] == 1;
}

// a dynamic-Huffman block header at bit b (ParallelGunzip::dynamic_header_at restated: BFINAL = 0, BTYPE = 2, a complete code-length
// code, a complete literal/length code with an end-of-block code, a distance code that is complete or a single code)
__device__ bool dyn_header_at(const uint8_t *d, uint64_t n, uint64_t b) {
    SlowBits r{d, n, b, true};
    if (r.get(1) != 0) return false;
    if (r.get(2) != 2) return false;
    const int hlit = (int)r.get(5) + 257, hdist = (int)r.get(5) + 1, hclen = (int)r.get(4) + 4;
    if (!r.ok || hlit > 286 || hdist > 30) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < hclen; ++i) cl[order[i]] = (uint8_t)r.get(3);
    if (!r.ok) return false;
    int count[16], nz = 0;
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < 19; ++i) { count[cl[i]]++; nz += cl[i] != 0; }
    if (!dg_complete(count, nz, 7, false, 19)) return false;
    int offs[8], symbol[19];
    offs[1] = 0;
    for (int l = 1; l < 7; ++l) offs[l + 1] = offs[l] + count[l];
    for (int i = 0; i < 19; ++i) if (cl[i]) symbol[offs[cl[i]]++] = i;
    int lc[16], dc[16], lnz = 0, dnz = 0, prev = -1;
    bool eob = false;
    for (int l = 0; l < 16; ++l) lc[l] = dc[l] = 0;
    int i = 0;
    const int total = hlit + hdist;
    while (i < total) {
        int code = 0, first = 0, index = 0, s = -1;
        for (int l = 1; l <= 7; ++l) {
            code |= (int)r.get(1);
            const int c = count[l];
            if (code - c < first) { s = symbol[index + (code - first)]; break; }
            index += c; first += c; first <<= 1; code <<= 1;
        }
        if (s < 0 || !r.ok) return false;
        int val, rep;
        if (s < 16) { val = s; rep = 1; }
        else if (s == 16) { if (i == 0) return false; val = prev; rep = 3 + (int)r.get(2); }
        else if (s == 17) { val = 0; rep = 3 + (int)r.get(3); }
        else { val = 0; rep = 11 + (int)r.get(7); }
        if (i + rep > total) return false;
        for (int k = 0; k < rep; ++k, ++i) {
            if (i < hlit) { lc[val]++; lnz += val != 0; if (i == 256) eob = val != 0; }
            else { dc[val]++; dnz += val != 0; }
        }
        prev = val;
    }
    if (!r.ok || !eob) return false;
    if (!dg_complete(lc, lnz, 15, false, hlit)) return false;
    if (!dg_complete(dc, dnz, 15, true, hdist)) return false;
    return true;
}

__global__ __launch_bounds__(256) void gzd_find_starts_kernel(const uint8_t *__restrict__ in, uint64_t in_len, int at_end, uint64_t first_cut, uint64_t chunk,
                                                              uint64_t lim, unsigned long long *__restrict__ starts) {
    __shared__ unsigned long long best;
    const uint64_t lo = first_cut + (uint64_t)blockIdx.x * chunk, hi = min(lo + chunk, lim);
    if (threadIdx.x == 0) best = NONE;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += blockDim.x) {
        const uint64_t by = base + threadIdx.x;
        if (by < hi) {
            for (int k = 0; k < 8; ++k) {
                const uint64_t b = 8 * by + k;
                bool ok = false;
                if (k == 0 && in[by] == 0x1f) ok = gz_header_len(in, in_len, by, at_end != 0) > 0;
                if (!ok) {
                    // cheap prefix test first: BFINAL = 0, BTYPE = 10b  ->  bits 0, 0, 1
                    const uint32_t w = (uint32_t)in[by] | ((by + 1 < in_len ? (uint32_t)in[by + 1] : 0u) << 8);
                    if (((w >> k) & 7u) == 4u) ok = dyn_header_at(in, in_len, b);
                }
                if (ok) { atomicMin(&best, (unsigned long long)b); break; }
            }
        }
        __syncthreads();
        const bool found = best != NONE;
        __syncthreads();
        if (found) break;
    }
    if (threadIdx.x == 0) {
        unsigned long long s = best;
        if (s != NONE && (s & 7) == 0) {
            const long h = gz_header_len(in, in_len, s >> 3, at_end != 0);
            if (h > 0) s = 8 * ((s >> 3) + (uint64_t)h);              // a member's first block: after its header
        }
        starts[blockIdx.x] = s;
    }
}

// ---- the decoder ----------------------------------------------------------------------------------------------------------
struct BitIn {
    const uint32_t *w;
    uint64_t nw;            // readable words (the buffer is padded; words past it read as 0)
    uint64_t bb, wi;
    uint32_t bc;
    __device__ void fill() { const uint64_t v = wi < nw ? w[wi] : 0u; bb |= v << bc; bc += 32; ++wi; }
    __device__ void init(uint64_t bit) { wi = bit >> 5; bb = 0; bc = 0; fill(); fill(); drop((uint32_t)(bit & 31)); }
    __device__ void need(uint32_t n) { if (bc < n) fill(); }      // n <= 32
    __device__ uint32_t peek(uint32_t n) const { return (uint32_t)(bb & ((1ull << n) - 1)); }
    __device__ void drop(uint32_t n) { bb >>= n; bc -= n; }
    __device__ uint32_t get(uint32_t n) { need(n); const uint32_t v = peek(n); drop(n); return v; }
    __device__ uint64_t pos() const { return (wi << 5) - bc; }
};

struct Code {               // one Huffman code in LDS: primary table + canonical counts / symbols for the longer codes
    uint16_t *tab; uint16_t *cnt; uint16_t *sym; int tb, symbits;
};

// kind 0: code-length code (must be complete), 1: literal/length, 2: distance (zlib's inflate_table: over-subscribed is an error,
// incomplete only with a single code of length 1; an empty distance code is allowed)
__device__ bool dg_build(const uint8_t *lens, int n, const Code &c, uint16_t *offs, int kind) {
    for (int l = 0; l < 16; ++l) c.cnt[l] = 0;
    for (int i = 0; i < n; ++i) c.cnt[lens[i]]++;
    int max = 15;
    while (max >= 1 && c.cnt[max] == 0) --max;
    for (int k = 0; k < (1 << c.tb); ++k) c.tab[k] = 0;
    if (max == 0) return kind == 2;
    int left = 1;
    for (int l = 1; l <= 15; ++l) { left <<= 1; left -= c.cnt[l]; if (left < 0) return false; }
    if (left > 0 && (kind == 0 || max != 1)) return false;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + c.cnt[l];
    for (int i = 0; i < n; ++i) if (lens[i]) c.sym[offs[lens[i]]++] = (uint16_t)i;
    uint32_t code = 0;
    int idx = 0;
    for (int len = 1; len <= 15; ++len) {
        for (int q = 0; q < c.cnt[len]; ++q, ++idx, ++code) {
            if (len > c.tb) continue;
            const uint32_t rev = __brev(code) >> (32 - len);
            const uint16_t e = (uint16_t)((len << c.symbits) | c.sym[idx]);
            for (uint32_t k = rev; k < (1u << c.tb); k += 1u << len) c.tab[k] = e;
        }
        code <<= 1;
    }
    return true;
}

// next symbol (the bit buffer holds >= 15 bits); -1: not a code
__device__ __forceinline__ int dg_decode(BitIn &in, const Code &c) {
    const uint32_t e = c.tab[in.bb & ((1u << c.tb) - 1)];
    if (e) { in.drop(e >> c.symbits); return (int)(e & ((1u << c.symbits) - 1)); }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((in.bb >> (len - 1)) & 1);
        const int cn = c.cnt[len];
        if (code - cn < first) { in.drop(len); return c.sym[index + (code - first)]; }
        index += cn; first += cn; first <<= 1; code <<= 1;
    }
    return -1;
}

__device__ const uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };

// One wave per candidate start; lane 0 walks the bits and writes the symbols (the wave's other lanes fill the length tables).
// in: the slab's compressed bytes (word-aligned), in_len valid bytes, at_end: they reach the end of the file.
__global__ __launch_bounds__(64) void gzd_decode_kernel(const uint8_t *__restrict__ in, uint64_t in_len, uint64_t in_words, int at_end,
                                                        const unsigned long long *__restrict__ cand, uint32_t ncand, uint64_t nominal_end_bit,
                                                        uint16_t *__restrict__ arena, uint64_t stride, uint64_t cap, GzdRec *__restrict__ recs) {
    __shared__ uint16_t s_lit[1 << LIT_BITS], s_dist[1 << DIST_BITS];
    __shared__ uint16_t s_lcnt[16], s_lsym[288], s_dcnt[16], s_dsym[32], s_offs[16];
    __shared__ uint8_t s_lens[320];
    __shared__ uint16_t s_lbase[29], s_dbase[30];
    __shared__ uint8_t s_lext[29], s_dext[30];
    const uint32_t d = blockIdx.x;
    if (threadIdx.x < 29) { s_lbase[threadIdx.x] = LBASE[threadIdx.x]; s_lext[threadIdx.x] = LEXT[threadIdx.x]; }
    if (threadIdx.x < 30) { s_dbase[threadIdx.x] = DBASE[threadIdx.x]; s_dext[threadIdx.x] = DEXT[threadIdx.x]; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    GzdRec *rec = recs + d;
    uint16_t *out = arena + (uint64_t)d * stride;
    const Code lit{s_lit, s_lcnt, s_lsym, LIT_BITS, 9}, dist{s_dist, s_dcnt, s_dsym, DIST_BITS, 5};
    const uint64_t in_bits = 8 * in_len;
    BitIn br{reinterpret_cast<const uint32_t *>(in), in_words, 0, 0, 0};
    uint64_t start = cand[d];
    br.init(start);
    uint32_t j = d + 1;                          // next candidate not behind the position
    uint64_t pos = 0;                            // symbols written
    int64_t mstart = -((int64_t)1 << 40);        // output offset where the current member began (far before: it began before the chunk)
    uint32_t nm = 0;
    uint64_t last_b = start, last_pos = 0;       // the last block start reached (where a gap would begin)
    uint32_t last_nm = 0;
    int fixed_built = 0;
    int status = GZ_ERR;
    uint64_t end_bit = 0;
    auto ran_out = [&]() { status = at_end ? GZ_ERR : GZ_GAP; };
    for (;;) {
        // ---- a block starts at br.pos() ----
        if (br.pos() > in_bits) { ran_out(); break; }
        const uint32_t hdr = br.get(3);
        const uint32_t bfinal = hdr & 1, btype = hdr >> 1;
        bool bad = false, full = false;
        if (btype == 0) {                                                       // stored
            br.drop(br.bc & 7);
            const uint32_t len = br.get(16), nlen = br.get(16);
            if (len != (~nlen & 0xFFFFu)) { status = GZ_ERR; break; }
            if (pos + len > cap) { status = GZ_GAP; break; }
            for (uint32_t k = 0; k < len; ++k) out[pos + k] = (uint16_t)br.get(8);
            pos += len;
        } else if (btype == 3) { status = GZ_ERR; break; }
        else {
            if (btype == 1) {
                if (!fixed_built) {
                    for (int i = 0; i < 288; ++i) s_lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                    dg_build(s_lens, 288, lit, s_offs, 1);
                    for (int i = 0; i < 32; ++i) s_lens[i] = 5;
                    dg_build(s_lens, 32, dist, s_offs, 2);
                    fixed_built = 1;
                }
            } else {
                fixed_built = 0;
                const int hlit = (int)br.get(5) + 257, hdist = (int)br.get(5) + 1, hclen = (int)br.get(4) + 4;
                if (hlit > 286 || hdist > 30) { status = GZ_ERR; break; }
                const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                for (int i = 0; i < 19; ++i) s_lens[i] = 0;
                for (int i = 0; i < hclen; ++i) s_lens[order[i]] = (uint8_t)br.get(3);
                const Code clc{s_lit, s_lcnt, s_lsym, 7, 9};
                if (!dg_build(s_lens, 19, clc, s_offs, 0)) { status = GZ_ERR; break; }
                const int total = hlit + hdist;
                int i = 0;
                uint8_t prev = 0;
                // (the code-length code was built into s_lit's storage: the lengths it decodes may overwrite its own in s_lens)
                uint8_t *L = s_lens;
                while (i < total) {
                    br.need(32);
                    const int s = dg_decode(br, clc);
                    if (s < 0) { bad = true; break; }
                    if (s < 16) { L[i++] = (uint8_t)s; prev = (uint8_t)s; continue; }
                    int rep;
                    uint8_t val = 0;
                    if (s == 16) { if (i == 0) { bad = true; break; } val = prev; rep = 3 + (int)br.get(2); }
                    else if (s == 17) rep = 3 + (int)br.get(3);
                    else rep = 11 + (int)br.get(7);
                    if (i + rep > total) { bad = true; break; }
                    for (int k = 0; k < rep; ++k) L[i++] = val;
                    prev = val;
                }
                if (bad) { status = GZ_ERR; break; }
                if (L[256] == 0) { status = GZ_ERR; break; }                      // no end-of-block code
                if (!dg_build(L, hlit, lit, s_offs, 1)) { status = GZ_ERR; break; }
                if (!dg_build(L + hlit, hdist, dist, s_offs, 2)) { status = GZ_ERR; break; }
            }
            // ---- literal / length symbols up to the end-of-block code ----
            for (;;) {
                br.need(32);
                const int s = dg_decode(br, lit);
                if (s < 0) { bad = true; break; }
                if (s < 256) {
                    if (pos >= cap) { full = true; break; }
                    out[pos++] = (uint16_t)s;
                    continue;
                }
                if (s == 256) break;
                const int li = s - 257;
                if (li >= 29) { bad = true; break; }
                const uint32_t len = s_lbase[li] + br.get(s_lext[li]);
                br.need(32);
                const int ds = dg_decode(br, dist);
                if (ds < 0 || ds >= 30) { bad = true; break; }
                const uint32_t dd = s_dbase[ds] + br.get(s_dext[ds]);
                if ((int64_t)pos - mstart < (int64_t)dd) { bad = true; break; }          // too far back: before the member's start
                if (pos + len > cap) { full = true; break; }
                const int64_t src = (int64_t)pos - (int64_t)dd;
                if (src >= 0 && dd >= 8) {
                    for (uint32_t k = 0; k < len; k += 8)
                        *reinterpret_cast<V16 *>(out + pos + k) = *reinterpret_cast<const V16 *>(out + src + k);
                } else if (src >= 0) {
                    // a period of dd < 8 symbols, all of them before pos
                    uint16_t p0 = out[src], p1 = dd > 1 ? out[src + 1] : 0, p2 = dd > 2 ? out[src + 2] : 0, p3 = dd > 3 ? out[src + 3] : 0,
                             p4 = dd > 4 ? out[src + 4] : 0, p5 = dd > 5 ? out[src + 5] : 0, p6 = dd > 6 ? out[src + 6] : 0;
                    uint32_t r = 0;
                    for (uint32_t k = 0; k < len; ++k) {
                        const uint16_t v = r == 0 ? p0 : r == 1 ? p1 : r == 2 ? p2 : r == 3 ? p3 : r == 4 ? p4 : r == 5 ? p5 : p6;
                        out[pos + k] = v;
                        if (++r == dd) r = 0;
                    }
                } else {
                    for (uint32_t k = 0; k < len; ++k) {
                        const int64_t q = src + (int64_t)k;
                        out[pos + k] = q >= 0 ? out[q] : (uint16_t)(256 + (int64_t)GZ_WIN + q);
                    }
                }
                pos += len;
            }
            if (bad) { status = GZ_ERR; break; }
        }
        if (full) { status = GZ_GAP; break; }
        uint64_t b = br.pos();
        if (b > in_bits) { ran_out(); break; }
        if (bfinal) {
            // ---- end of a member: trailer, then the next member's header or the end of the file ----
            uint64_t by = (b + 7) >> 3;
            if (by + 8 > in_len) { ran_out(); break; }
            if (nm == GZ_MAXM) { status = GZ_GAP; break; }
            const uint32_t crc = in[by] | (in[by + 1] << 8) | (in[by + 2] << 16) | ((uint32_t)in[by + 3] << 24);
            const uint32_t isz = in[by + 4] | (in[by + 5] << 8) | (in[by + 6] << 16) | ((uint32_t)in[by + 7] << 24);
            rec->m_off[nm] = pos;
            rec->m_crc[nm] = crc;
            rec->m_isize[nm] = isz;
            ++nm;
            mstart = (int64_t)pos;
            by += 8;
            while (by < in_len && in[by] == 0) ++by;                 // (zero padding between members, as gzip tolerates)
            if (by >= in_len) {
                if (at_end) { status = GZ_EOF; end_bit = 8 * in_len; last_pos = pos; last_nm = nm; }
                else status = GZ_GAP;
                break;
            }
            const long h = gz_header_len(in, in_len, by, at_end != 0);
            if (h == 0) { status = GZ_ERR; break; }                  // trailing garbage (the many-thread reader's verdict)
            if (h < 0) { status = GZ_GAP; break; }
            b = 8 * (by + (uint64_t)h);
            br.init(b);
        }
        // ---- a block boundary: stop at a later candidate's start or past the slab's end ----
        while (j < ncand && cand[j] < b) ++j;
        if (j < ncand && cand[j] == b) { status = GZ_STOP; end_bit = b; last_pos = pos; last_nm = nm; break; }
        if (b >= nominal_end_bit) { status = GZ_SLAB_END; end_bit = b; last_pos = pos; last_nm = nm; break; }
        last_b = b; last_pos = pos; last_nm = nm;
    }
    if (status == GZ_GAP) end_bit = last_b;
    rec->status = (unsigned)status;
    rec->end_bit = end_bit;
    rec->out_len = last_pos;
    rec->n_members = last_nm;
}

// One workgroup walks the accepted chunks in order with the 32 KB window in LDS: writes the window before each chunk, then moves
// it past the chunk (its last 32 KB of symbols, resolved against the window before it).
// acc: per accepted chunk {decoder, symbols, text offset, valid window bytes}
__global__ __launch_bounds__(1024) void gzd_window_kernel(const uint16_t *__restrict__ arena, uint64_t stride, const unsigned long long *__restrict__ acc, uint32_t n_acc,
                                                          uint8_t *__restrict__ win_carry, uint8_t *__restrict__ wins) {
    __shared__ uint8_t wa[GZ_WIN], wb[GZ_WIN];
    uint8_t *cw = wa, *nw = wb;
    for (uint32_t i = threadIdx.x * 16; i < GZ_WIN; i += blockDim.x * 16)
        *reinterpret_cast<uint4 *>(cw + i) = *reinterpret_cast<const uint4 *>(win_carry + i);
    __syncthreads();
    for (uint32_t c = 0; c < n_acc; ++c) {
        const uint64_t dsel = acc[4 * c], L = acc[4 * c + 1];
        const uint16_t *S = arena + dsel * stride;
        for (uint32_t i = threadIdx.x * 16; i < GZ_WIN; i += blockDim.x * 16)
            *reinterpret_cast<uint4 *>(wins + (uint64_t)c * GZ_WIN + i) = *reinterpret_cast<const uint4 *>(cw + i);
        for (uint32_t i = threadIdx.x; i < GZ_WIN; i += blockDim.x) {
            uint8_t v;
            if (L >= GZ_WIN) { const uint16_t s = S[L - GZ_WIN + i]; v = s < 256 ? (uint8_t)s : cw[(s - 256) & (GZ_WIN - 1)]; }
            else if (i < GZ_WIN - L) v = cw[i + L];
            else { const uint16_t s = S[i - (GZ_WIN - L)]; v = s < 256 ? (uint8_t)s : cw[(s - 256) & (GZ_WIN - 1)]; }
            nw[i] = v;
        }
        __syncthreads();
        uint8_t *t = cw; cw = nw; nw = t;
    }
    for (uint32_t i = threadIdx.x * 16; i < GZ_WIN; i += blockDim.x * 16)
        *reinterpret_cast<uint4 *>(win_carry + i) = *reinterpret_cast<const uint4 *>(cw + i);
}

// final bytes in stitched order: one workgroup per accepted chunk; a symbol of the window before the member's start is an error (*bad)
__global__ __launch_bounds__(256) void gzd_resolve_kernel(const uint16_t *__restrict__ arena, uint64_t stride, const unsigned long long *__restrict__ acc,
                                                          const uint8_t *__restrict__ wins, uint8_t *__restrict__ text, unsigned int *__restrict__ bad) {
    const uint32_t c = blockIdx.x;
    const uint64_t dsel = acc[4 * c], L = acc[4 * c + 1], off = acc[4 * c + 2], valid = acc[4 * c + 3];
    const uint16_t *S = arena + dsel * stride;
    const uint8_t *W = wins + (uint64_t)c * GZ_WIN;
    const uint32_t lo_ok = (uint32_t)(GZ_WIN - valid);
    bool b = false;
    for (uint64_t i = (uint64_t)threadIdx.x * 8; i < L; i += (uint64_t)blockDim.x * 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(S + i);      // (the arena's rows are 16-byte aligned)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint8_t o[8];
        for (int k = 0; k < 8; ++k) {
            const uint32_t s = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            if (s < 256) o[k] = (uint8_t)s;
            else { const uint32_t p = (s - 256) & (GZ_WIN - 1); b |= p < lo_ok && i + k < L; o[k] = W[p]; }
        }
        if (i + 8 <= L) {
            struct __attribute__((packed, aligned(1))) V8 { uint32_t a, b; };
            V8 t;
            t.a = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
            t.b = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
            *reinterpret_cast<V8 *>(text + off + i) = t;
        } else {
            for (int k = 0; k < 8 && i + k < L; ++k) text[off + i + k] = o[k];
        }
    }
    if (b) atomicOr(bad, 1u);
}

// CRC-32 (zlib's) of every piece: one thread per piece
__global__ __launch_bounds__(256) void gzd_crc_kernel(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ poff, const unsigned int *__restrict__ plen,
                                                      uint32_t n, unsigned int *__restrict__ crc_out) {
    __shared__ uint32_t tab[256];
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        tab[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *p = text + poff[i];
    const uint32_t len = plen[i];
    uint32_t c = 0xFFFFFFFFu, k = 0;
    while (k < len && ((uintptr_t)(p + k) & 3)) { c = tab[(c ^ p[k]) & 0xFF] ^ (c >> 8); ++k; }
    for (; k + 4 <= len; k += 4) {
        uint32_t w = *reinterpret_cast<const uint32_t *>(p + k);
        for (int q = 0; q < 4; ++q) { c = tab[(c ^ w) & 0xFF] ^ (c >> 8); w >>= 8; }
    }
    for (; k < len; ++k) c = tab[(c ^ p[k]) & 0xFF] ^ (c >> 8);
    crc_out[i] = ~c;
}

// ---- CRC-32 combination on the host (GF(2) polynomial arithmetic, as in zlib 1.2.12's crc32_combine) ----------------------
uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
uint32_t x2nmodp(uint64_t n, unsigned k) {           // x^(n * 2^k) modulo p(x)
    struct Table { uint32_t t[32]; Table() { uint32_t p = 1u << 30; t[0] = p; for (int i = 1; i < 32; ++i) t[i] = p = multmodp(p, p); } };
    static const Table table;
    uint32_t p = 1u << 31;
    while (n) { if (n & 1) p = multmodp(table.t[k & 31], p); n >>= 1; ++k; }
    return p;
}
inline uint32_t crc_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return multmodp(x2nmodp(len2, 3), crc1) ^ crc2; }

size_t env_size(const char *name, size_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    return (size_t)strtoull(e, nullptr, 10);
}

struct Geometry {
    size_t slab, ncuts_max, n_dec_max, cap, stride, in_cap, text_cap, pieces_max;
};
Geometry geometry(size_t file_bytes, const GzdConfig &cfg) {
    Geometry g;
    g.slab = std::min(cfg.slab, (file_bytes + 4095) / 4096 * 4096 + 4096);
    g.ncuts_max = g.slab / cfg.chunk + 2;
    g.n_dec_max = (cfg.false_starts ? 2 : 1) * g.ncuts_max + 2;
    g.cap = 16 * cfg.chunk;                                   // symbols per decoder (reads compress 3-8x: room for running past a false start)
    g.stride = g.cap + 16;                                    // (16-byte copies may write up to 7 symbols past the end)
    g.in_cap = g.slab + GZ_MARGIN + 8192 + 64;
    g.text_cap = g.n_dec_max * g.cap + 64;
    g.pieces_max = g.text_cap / GZ_PIECE + g.n_dec_max * (GZ_MAXM + 2) + 16;
    return g;
}
size_t small_bytes(const Geometry &g) {
    return g.ncuts_max * 8 + g.n_dec_max * 8 + g.n_dec_max * sizeof(GzdRec) + g.n_dec_max * 32 + g.pieces_max * 16 + 256;
}

}  // namespace

GzdConfig GzdConfig::from_env() {
    GzdConfig c;
    c.chunk = std::max<size_t>(4096, env_size("JASPER_INGEST_GZ_DEVICE_CHUNK", c.chunk));
    c.slab = std::max<size_t>(4 * c.chunk, std::max<size_t>(1u << 20, env_size("JASPER_INGEST_GZ_DEVICE_SLAB_MB", c.slab >> 20) << 20));
    const char *f = getenv("JASPER_INGEST_GZ_DEVICE_FALSE_STARTS");
    c.false_starts = f && atoi(f) != 0;
    return c;
}

size_t DeviceGunzip::bytes_needed(int slot, size_t file_bytes, const GzdConfig &cfg) {
    const Geometry g = geometry(file_bytes, cfg);
    switch (slot) {
    case 0: return g.in_cap;
    case 1: return g.n_dec_max * g.stride * 2;
    case 2: return g.text_cap;
    case 3: return (g.n_dec_max + 1) * (size_t)GZ_WIN;
    default: return small_bytes(g);
    }
}

DeviceGunzip::DeviceGunzip(const char *path, int device, hipStream_t stream, const GzdConfig &cfg, uint64_t *stats)
    : path_(path), device_(device), stream_(stream), cfg_(cfg), stats_(stats) {}

DeviceGunzip::~DeviceGunzip() {
    if (data_) munmap((void *)data_, n_);
    if (fd_ >= 0) ::close(fd_);
}

bool DeviceGunzip::open(const Alloc &alloc) {
    fd_ = ::open(path_.c_str(), O_RDONLY);
    if (fd_ < 0) return false;
    struct stat st;
    if (fstat(fd_, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 18) return false;
    n_ = (size_t)st.st_size;
    void *m = mmap(nullptr, n_, PROT_READ, MAP_PRIVATE, fd_, 0);
    if (m == MAP_FAILED) { n_ = 0; return false; }
    data_ = (const uint8_t *)m;
    (void)madvise(m, n_, MADV_SEQUENTIAL);
    const long h = gz_header_len(data_, n_, 0, true);
    if (h <= 0) return false;
    const Geometry g = geometry(n_, cfg_);
    void *p[N_SLOTS];
    for (int s = 0; s < N_SLOTS; ++s) {
        p[s] = alloc(s, bytes_needed(s, n_, cfg_));
        if (!p[s]) return false;
    }
    d_in_ = (uint8_t *)p[0];
    d_arena_ = (uint16_t *)p[1];
    d_text_ = (uint8_t *)p[2];
    d_wins_ = (uint8_t *)p[3];
    d_small_ = (uint8_t *)p[4];
    in_cap_ = g.in_cap; cap_ = g.cap; n_dec_max_ = g.n_dec_max; ncuts_max_ = g.ncuts_max; text_cap_ = g.text_cap; pieces_max_ = g.pieces_max;
    cur_bit_ = 8ull * (uint64_t)h;
    win_valid_ = 0;
    win_.assign(GZ_WIN, 0);
    if (hipSetDevice(device_) != hipSuccess) return false;
    // the window before the stream: nothing (win carry lives after the per-chunk windows)
    if (hipMemsetAsync(d_wins_ + n_dec_max_ * (size_t)GZ_WIN, 0, GZ_WIN, stream_) != hipSuccess) return false;
    return true;
}

bool DeviceGunzip::member_end(uint32_t crc, uint32_t isize) {
    if (crc_ != crc || (uint32_t)member_len_ != isize) { err = "crc or length error in " + path_; return false; }
    crc_ = 0;
    member_len_ = 0;
    if (stats_) stats_[GZS_MEMBERS]++;
    return true;
}

void DeviceGunzip::keep_window(const uint8_t *p, size_t n) {
    if (n >= GZ_WIN) { memcpy(win_.data(), p + n - GZ_WIN, GZ_WIN); return; }
    memmove(win_.data(), win_.data() + n, GZ_WIN - n);
    memcpy(win_.data() + GZ_WIN - n, p, n);
}

// zlib from start_bit (a block start; the window: win_, its last win_valid_ bytes belong to the member) to the first block start at or
// past stop_bit, or the end of the stream.  Member ends are checked here; the text is appended to out.
bool DeviceGunzip::host_fill(uint64_t start_bit, uint64_t stop_bit, std::vector<uint8_t> &out, uint64_t &end_bit, bool &eof) {
    z_stream s;
    memset(&s, 0, sizeof s);
    if (inflateInit2(&s, -15) != Z_OK) { err = "zlib"; return false; }
    size_t by = (size_t)(start_bit >> 3);
    const int bit = (int)(start_bit & 7);
    if (bit) { inflatePrime(&s, 8 - bit, data_[by] >> bit); ++by; }
    if (win_valid_) inflateSetDictionary(&s, win_.data() + GZ_WIN - win_valid_, (uInt)win_valid_);
    const size_t base = out.size();
    size_t produced = base, mark = base;          // mark: where the current member's text in out begins (for its CRC)
    out.resize(base + (16u << 20));
    s.next_in = const_cast<Bytef *>(data_ + by);
    size_t in_left = n_ - by;
    s.avail_in = (uInt)std::min<size_t>(in_left, 1u << 30);
    in_left -= s.avail_in;
    bool ok = false;
    eof = false;
    for (;;) {
        if (produced == out.size()) out.resize(out.size() + out.size() / 2);
        s.next_out = out.data() + produced;
        const size_t room = std::min<size_t>(out.size() - produced, 1u << 30);
        s.avail_out = (uInt)room;
        if (s.avail_in == 0 && in_left) { s.avail_in = (uInt)std::min<size_t>(in_left, 1u << 30); in_left -= s.avail_in; }
        const int rc = inflate(&s, Z_BLOCK);
        produced += room - s.avail_out;
        if (rc == Z_STREAM_END) {
            size_t pos = (size_t)(s.next_in - data_);
            if (pos + 8 > n_) { err = "read error in " + path_; break; }
            const uint32_t crc = data_[pos] | (data_[pos + 1] << 8) | (data_[pos + 2] << 16) | ((uint32_t)data_[pos + 3] << 24);
            const uint32_t isz = data_[pos + 4] | (data_[pos + 5] << 8) | (data_[pos + 6] << 16) | ((uint32_t)data_[pos + 7] << 24);
            crc_ = (uint32_t)crc32(crc_, out.data() + mark, (uInt)(produced - mark));
            member_len_ += produced - mark;
            mark = produced;
            if (!member_end(crc, isz)) break;
            pos += 8;
            while (pos < n_ && data_[pos] == 0) ++pos;
            if (pos >= n_) { eof = true; end_bit = 8ull * n_; ok = true; break; }
            const long h = gz_header_len(data_, n_, pos, true);
            if (h <= 0) { err = "read error in " + path_; break; }
            const uint64_t nb = 8ull * (pos + (size_t)h);
            if (nb >= stop_bit) { end_bit = nb; ok = true; break; }
            inflateReset2(&s, -15);
            s.next_in = const_cast<Bytef *>(data_ + pos + h);
            in_left = n_ - (pos + h);
            s.avail_in = (uInt)std::min<size_t>(in_left, 1u << 30);
            in_left -= s.avail_in;
            continue;
        }
        if (rc != Z_OK && rc != Z_BUF_ERROR) { err = "read error in " + path_; break; }
        if (rc == Z_BUF_ERROR && s.avail_in == 0 && in_left == 0 && s.avail_out != 0) { err = "read error in " + path_; break; }
        if ((s.data_type & 128) && !(s.data_type & 64)) {
            const uint64_t posb = 8ull * (uint64_t)(s.next_in - data_) - (uint64_t)(s.data_type & 63);
            if (posb >= stop_bit) { end_bit = posb; ok = true; break; }
        }
    }
    inflateEnd(&s);
    if (!ok) return false;
    // the rest of the member's text so far
    crc_ = (uint32_t)crc32(crc_, out.data() + mark, (uInt)(produced - mark));
    member_len_ += produced - mark;
    win_valid_ = std::min<size_t>(GZ_WIN, (mark == base ? win_valid_ : 0) + (produced - mark));
    out.resize(produced);
    keep_window(out.data() + base, produced - base);
    return true;
}

#define GZCHK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return false; } \
    } while (0)

bool DeviceGunzip::next_slab() {
    const uint64_t cur_byte = cur_bit_ >> 3;
    const uint64_t base = cur_byte & ~(uint64_t)4095;
    const uint64_t hi = std::min<uint64_t>(n_, cur_byte + cfg_.slab);          // nominal end (bytes)
    const uint64_t buf_end = std::min<uint64_t>(n_, hi + GZ_MARGIN);
    const bool at_end = buf_end == n_;
    const uint64_t in_len = buf_end - base;
    const uint64_t rel_cur = cur_bit_ - 8 * base, nominal_end_bit = 8 * (hi - base);
    if (stats_) stats_[GZS_SLABS]++;
    GZCHK(hipMemcpyAsync(d_in_, data_ + base, in_len, hipMemcpyHostToDevice, stream_));
    GZCHK(hipMemsetAsync(d_in_ + in_len, 0, 64, stream_));
    unsigned long long *d_starts = (unsigned long long *)d_small_;
    unsigned long long *d_cand = d_starts + ncuts_max_;
    GzdRec *d_recs = (GzdRec *)(d_cand + n_dec_max_);
    unsigned long long *d_acc = (unsigned long long *)(d_recs + n_dec_max_);
    unsigned long long *d_poff = d_acc + 4 * n_dec_max_;
    unsigned int *d_plen = (unsigned int *)(d_poff + pieces_max_);
    unsigned int *d_pcrc = d_plen + pieces_max_;
    unsigned int *d_bad = d_pcrc + pieces_max_;
    uint8_t *d_carry = d_wins_ + n_dec_max_ * (size_t)GZ_WIN;
    // 1. candidate starts
    const uint64_t first_cut = cur_byte - base + cfg_.chunk;
    const uint64_t lim = hi - base;
    uint32_t ncuts = 0;
    if (first_cut < lim) ncuts = (uint32_t)std::min<uint64_t>((lim - first_cut + cfg_.chunk - 1) / cfg_.chunk, ncuts_max_);
    std::vector<unsigned long long> starts(ncuts);
    if (ncuts) {
        hipLaunchKernelGGL(gzd_find_starts_kernel, dim3(ncuts), dim3(256), 0, stream_, d_in_, in_len, at_end ? 1 : 0, first_cut, (uint64_t)cfg_.chunk, lim, d_starts);
        GZCHK(hipGetLastError());
        GZCHK(hipMemcpyAsync(starts.data(), d_starts, ncuts * 8, hipMemcpyDeviceToHost, stream_));
        GZCHK(hipStreamSynchronize(stream_));
    }
    std::vector<unsigned long long> cand;
    cand.push_back(rel_cur);
    for (unsigned long long s : starts) if (s != NONE && s > rel_cur && s < nominal_end_bit) cand.push_back(s);
    std::sort(cand.begin() + 1, cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    if (cfg_.false_starts) {                  // test hook: a bogus start in the middle of every chunk
        const size_t nreal = cand.size();
        for (size_t i = 0; i < nreal; ++i) {
            const uint64_t a = cand[i], b = i + 1 < nreal ? cand[i + 1] : std::min<uint64_t>(nominal_end_bit, a + 8 * cfg_.chunk);
            if (b > a + 2) cand.push_back(a + (b - a) / 2 + 1);
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    }
    if (cand.size() > n_dec_max_) cand.resize(n_dec_max_);
    const uint32_t ncand = (uint32_t)cand.size();
    if (stats_) stats_[GZS_DECODERS] += ncand;
    // 2. decoders
    GZCHK(hipMemcpyAsync(d_cand, cand.data(), ncand * 8, hipMemcpyHostToDevice, stream_));
    const uint64_t stride = cap_ + 16;
    hipLaunchKernelGGL(gzd_decode_kernel, dim3(ncand), dim3(64), 0, stream_, d_in_, in_len, (in_len + 64) / 4, at_end ? 1 : 0, d_cand, ncand, nominal_end_bit,
                       d_arena_, stride, (uint64_t)cap_, d_recs);
    GZCHK(hipGetLastError());
    std::vector<GzdRec> recs(ncand);
    GZCHK(hipMemcpyAsync(recs.data(), d_recs, ncand * sizeof(GzdRec), hipMemcpyDeviceToHost, stream_));
    GZCHK(hipStreamSynchronize(stream_));
    // 3. stitch: the chain from the slab's first chunk
    std::vector<unsigned long long> acc;       // {decoder, symbols, text offset, valid window bytes}
    struct MEnd { uint64_t text_off; uint32_t crc, isize; };
    std::vector<MEnd> mends;
    uint64_t T = 0;
    size_t valid = win_valid_;
    bool gap = false, done_eof = false;
    uint64_t next_bit = 0;
    uint32_t i = 0;
    for (;;) {
        const GzdRec &r = recs[i];
        if (r.status == GZ_ERR) { err = "read error in " + path_; return false; }
        if (r.out_len) {
            acc.push_back(i); acc.push_back(r.out_len); acc.push_back(T); acc.push_back(valid);
        }
        for (uint32_t m = 0; m < r.n_members; ++m) mends.push_back({T + r.m_off[m], r.m_crc[m], r.m_isize[m]});
        if (r.n_members) valid = std::min<uint64_t>(GZ_WIN, r.out_len - r.m_off[r.n_members - 1]);
        else valid = std::min<uint64_t>(GZ_WIN, valid + r.out_len);
        T += r.out_len;
        if (r.status == GZ_STOP) {
            const auto it = std::lower_bound(cand.begin(), cand.end(), r.end_bit);
            if (it == cand.end() || *it != r.end_bit) { err = "inflate: chain broken in " + path_; return false; }
            i = (uint32_t)(it - cand.begin());
            continue;
        }
        next_bit = r.end_bit;
        if (r.status == GZ_EOF) done_eof = true;
        else if (r.status == GZ_GAP) gap = true;
        break;
    }
    const uint32_t n_acc = (uint32_t)(acc.size() / 4);
    if (stats_) { stats_[GZS_ACCEPTED] += n_acc; stats_[GZS_DEVICE_BYTES] += T; }
    // 4-5. windows, bytes, CRC pieces
    std::vector<unsigned long long> poff;
    std::vector<unsigned int> plen;
    std::vector<int64_t> events;               // >= 0: piece index; < 0: member end -(m + 1)
    {
        uint64_t at = 0;
        auto pieces_to = [&](uint64_t upto) {
            while (at < upto) {
                const uint64_t l = std::min<uint64_t>(GZ_PIECE, upto - at);
                events.push_back((int64_t)poff.size());
                poff.push_back(at); plen.push_back((unsigned)l);
                at += l;
            }
        };
        for (size_t m = 0; m < mends.size(); ++m) { pieces_to(mends[m].text_off); events.push_back(-(int64_t)m - 1); }
        pieces_to(T);
    }
    if (poff.size() > pieces_max_) { err = "inflate: too many pieces"; return false; }
    std::vector<unsigned int> pcrc(poff.size());
    unsigned int bad = 0;
    if (n_acc) {
        if (T > text_cap_) { err = "inflate: text buffer"; return false; }
        GZCHK(hipMemcpyAsync(d_acc, acc.data(), acc.size() * 8, hipMemcpyHostToDevice, stream_));
        GZCHK(hipMemsetAsync(d_bad, 0, 4, stream_));
        hipLaunchKernelGGL(gzd_window_kernel, dim3(1), dim3(1024), 0, stream_, d_arena_, stride, d_acc, n_acc, d_carry, d_wins_);
        hipLaunchKernelGGL(gzd_resolve_kernel, dim3(n_acc), dim3(256), 0, stream_, d_arena_, stride, d_acc, d_wins_, d_text_, d_bad);
        GZCHK(hipGetLastError());
        if (!poff.empty()) {
            GZCHK(hipMemcpyAsync(d_poff, poff.data(), poff.size() * 8, hipMemcpyHostToDevice, stream_));
            GZCHK(hipMemcpyAsync(d_plen, plen.data(), plen.size() * 4, hipMemcpyHostToDevice, stream_));
            hipLaunchKernelGGL(gzd_crc_kernel, dim3((unsigned)((poff.size() + 255) / 256)), dim3(256), 0, stream_, d_text_, d_poff, d_plen, (uint32_t)poff.size(), d_pcrc);
            GZCHK(hipGetLastError());
            GZCHK(hipMemcpyAsync(pcrc.data(), d_pcrc, pcrc.size() * 4, hipMemcpyDeviceToHost, stream_));
        }
        GZCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream_));
    }
    if (gap) GZCHK(hipMemcpyAsync(win_.data(), d_carry, GZ_WIN, hipMemcpyDeviceToHost, stream_));     // the window where the gap begins
    GZCHK(hipStreamSynchronize(stream_));
    if (bad) { err = "read error in " + path_; return false; }
    static const uint32_t op_piece = x2nmodp(GZ_PIECE, 3);
    for (int64_t e : events) {
        if (e >= 0) {
            const uint32_t l = plen[(size_t)e];
            crc_ = (l == GZ_PIECE ? multmodp(op_piece, crc_) : multmodp(x2nmodp(l, 3), crc_)) ^ pcrc[(size_t)e];
            member_len_ += l;
        } else {
            const MEnd &m = mends[(size_t)(-e - 1)];
            if (!member_end(m.crc, m.isize)) return false;
        }
    }
    win_valid_ = valid;
    dev_text_n_ = T;
    dev_text_at_ = 0;
    host_text_.clear();
    host_text_at_ = 0;
    if (gap) {
        // the device gave up at next_bit: zlib on the host from there to the first block start past the slab's end
        uint64_t end_bit = 0;
        bool eof = false;
        if (!host_fill(8 * base + next_bit, 8 * hi, host_text_, end_bit, eof)) { if (err.empty()) err = "read error in " + path_; return false; }
        if (stats_) stats_[GZS_HOST_BYTES] += host_text_.size();
        GZCHK(hipMemcpyAsync(d_carry, win_.data(), GZ_WIN, hipMemcpyHostToDevice, stream_));
        GZCHK(hipStreamSynchronize(stream_));
        cur_bit_ = end_bit;
        eof_ = eof;
        return true;
    }
    cur_bit_ = 8 * base + next_bit;
    eof_ = done_eof;
    return true;
}

long DeviceGunzip::read(char *dst, size_t want) {
    if (!err.empty()) return -1;
    if (hipSetDevice(device_) != hipSuccess) { err = "hipSetDevice"; return -1; }
    size_t got = 0;
    while (got < want) {
        if (dev_text_at_ < dev_text_n_) {
            const size_t m = (size_t)std::min<uint64_t>(want - got, dev_text_n_ - dev_text_at_);
            hipError_t e = hipMemcpyAsync(dst + got, d_text_ + dev_text_at_, m, hipMemcpyDeviceToHost, stream_);
            if (e == hipSuccess) e = hipStreamSynchronize(stream_);
            if (e != hipSuccess) { err = std::string("inflate copy: ") + hipGetErrorString(e); return -1; }
            dev_text_at_ += m;
            got += m;
            continue;
        }
        if (host_text_at_ < host_text_.size()) {
            const size_t m = std::min(want - got, host_text_.size() - host_text_at_);
            memcpy(dst + got, host_text_.data() + host_text_at_, m);
            host_text_at_ += m;
            got += m;
            continue;
        }
        if (eof_) break;
        if (!next_slab()) { if (err.empty()) err = "read error in " + path_; return -1; }
    }
    return (long)got;
}

long DeviceGunzip::read_device(uint8_t *d_dst, size_t want) {
    if (!err.empty()) return -1;
    if (hipSetDevice(device_) != hipSuccess) { err = "hipSetDevice"; return -1; }
    size_t got = 0;
    while (got < want) {
        if (dev_text_at_ < dev_text_n_) {
            const size_t m = (size_t)std::min<uint64_t>(want - got, dev_text_n_ - dev_text_at_);
            const hipError_t e = hipMemcpyAsync(d_dst + got, d_text_ + dev_text_at_, m, hipMemcpyDeviceToDevice, stream_);
            if (e != hipSuccess) { err = std::string("inflate copy: ") + hipGetErrorString(e); return -1; }
            dev_text_at_ += m;
            got += m;
            continue;
        }
        if (host_text_at_ < host_text_.size()) {
            const size_t m = std::min(want - got, host_text_.size() - host_text_at_);
            hipError_t e = hipMemcpyAsync(d_dst + got, host_text_.data() + host_text_at_, m, hipMemcpyHostToDevice, stream_);
            if (e == hipSuccess) e = hipStreamSynchronize(stream_);      // (host_text_ is pageable and is cleared by the next slab)
            if (e != hipSuccess) { err = std::string("inflate copy: ") + hipGetErrorString(e); return -1; }
            host_text_at_ += m;
            got += m;
            continue;
        }
        if (eof_) break;
        if (!next_slab()) { if (err.empty()) err = "read error in " + path_; return -1; }      // (it waits for the stream: d_text_ is free to be written again)
    }
    return (long)got;
}

}  // namespace jk
