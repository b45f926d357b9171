// indels.hip -- indel scan: same-base insertions and deletions of up to 16 bytes that the reads hold against the sequence, as per-sequence
// counters and one record per hypothesis that is solid (semantics: include/jasper_hip.h, jasper_indel_scan); on request also the insertions
// of mixed bases (jasper_indel_scan_mixed).
//
// An extension.  The reference repairs such differences inside its walk (src/jasper.py: fix_insert, fix_del, fix_same_base_del,
// fix_same_base_insertion) and reports nothing.  The dense scan is that of variants.hip, unchanged: its candidate (p, x) -- the window
// that ends at p is solid with its last base replaced by x -- is window 0 of the alternative string of ins(p, x, L) and of del(p, L) with
// s[p + L] == x, hence necessary for all of them.
//
//   indels_check_kernel   one wave per candidate.  The wave loads the context bytes s[p-k+1 .. p+max_len+k-2] once (up to 142: lane l holds
//                         bytes l, l + 64 and l + 128; a byte past the sequence's end counts as "no base").  Nothing is evaluated unless
//                         the first 2k - 2 of them are bases (that is the condition of an insertion, and every deletion's includes it).
//                         Six ballots turn the context into two bit planes of three wave-uniform words.  A hypothesis is a VIRTUAL
//                         string -- the context with x^L put in before byte k - 1, or with L bytes taken out from there -- which is a
//                         few shifts and masks of those words in scalar registers; a lane cuts the window it owns out of the planes
//                         (a funnel shift, a bit reversal and an interleave per plane: no loop over the k bases, no shuffle).
//                           prefix   windows j < max_len of F + x^max_len, lane j.  Window j is shared by every ins(.., L > j), and window 0
//                                    is window 0 of every deletion.  The first one below thre bounds the L that can still pass; a prefix
//                                    minimum over the 16 lanes gives each L its part of alt_min.
//                           ins L    for L up to that bound: windows L .. k+L-2, lane j - L  (k - 1 lookups)
//                           del L    for every L with s[p + L] == x whose bytes are bases: windows 1 .. k-2  (k - 2 lookups)
//                           ref      only when a hypothesis passed: windows 0 .. k+L-2 of s for the largest deletion L that passed (k - 2
//                                    for insertions alone), lane j and, past 64, lane j - 64 a second one; looked up once, then one
//                                    masked minimum per hypothesis that passed.
//                         The hypotheses that passed are bits of a wave-uniform mask (bit L - 1: ins L, bit 15 + L: del L); lane b keeps
//                         the minima of bit b and writes its record.  Places are reserved with one returning cursor add per wave, and a
//                         wave writes all its records or none.
//
//   indels_mixed_kernel   (only when the caller asks for mixed insertions) one wave per candidate (p, x): a front search on the shared
//                         pieces of front_search.hpp over the inserted string y, y[0] == x.  The frontier S_t -- the
//                         prefixes of length t all of whose windows of F + y are solid -- is at most INDEL_FRONT = 64 prefixes, one per
//                         lane: y as 2-bit codes in a word (first base in the highest pair, so that lane order is lexicographic order)
//                         and the minimum over its t windows.  The kernel's own part of each shared step:
//                           rejoin   per level: window t of F + y + s[p ..], the first that holds s[p], lane i for its own prefix
//                                    (128-bit arithmetic on F's k-mer, one lookup per prefix that is not x^t); then front_rejoin with
//                                    windows t+1 .. k+t-2 cut out of the planes with y put in (pl_ins_y)
//                           ref      windows 0 .. k-2 of s, once per candidate and only when something passed
//                           records  (front_reserve) lane i its own.  Same-base strings x^t stay in the frontier but are never
//                                    written: they are the check's.
//                           extend   (front_extend, front_handover) the child's newest window is the last k bases of F + y + z; the
//                                    strip is 64 x 8 bytes per wave.  More than 64 children: the site is complex, counted once, and the
//                                    wave stops there.  Four lookups per prefix.
//
//   het_cluster_kernel    (only when the caller asks for het clusters, cluster_len = N > 0) one wave per candidate (p, x): the replacements
//                         of s[p .. p+R) by a string y, y[0] == x, R and |y| up to N, where the sequence and the replacement are both
//                         solid.  The wave loads the context s[p-k+1 .. p+N+k-2] (up to 190 bytes: lane l holds bytes l, l + 64, l + 128)
//                         and makes the two bit planes of it.
//                           ref      the reference windows 0 .. k+R-2 for the largest R whose bytes are bases, in at most two rounds
//                                    (k - 1 + N <= 127 windows: lane j, then lane j - 64).  After the first round a candidate whose own k
//                                    windows are not all solid leaves: R_max = 0, the compound scan's.  A prefix minimum over both rounds
//                                    puts ref_min(R) on lane R - 1, and the ballot of ref_min(R) >= thre is R_max (wave-uniform).
//                           lane R-1 keeps CW = the k - 1 bases before p + R (closure) and G = the k - 1 bases from p + R on (rejoin).
//                         Then a front search (front_search.hpp) with y in 128 bits (first base in the highest pair; the shift
//                         boundaries t < k, t >= k - 1 and t = 64 are those compound.hip documents), per level t:
//                           closure  per prefix, W = the last k - 1 bases of F + y against every lane's CW: one 128-bit compare, one ballot
//                           extend   (front_extend, front_handover) every prefix is looked up, the closed ones too: the four answers are
//                                    window t of F + y + G_R for the R with s[p+R] == z, so lane i keeps its prefix's 4-bit solid mask
//                                    from the round's ballot.  Only children of prefixes that are not closed enter the strip.
//                           rejoin   per prefix, lane R - 1: normal form and one bit of that mask (no lookup); the R that survive look up
//                                    windows t+1 .. t+3 one after the other, each lane its own, leaving at the first that fails -- every
//                                    one of them cuts the field to a quarter in ordinary sequence; what is left runs all k - 1 windows
//                                    t .. t+k-2 lane-parallel with a wave minimum, in a wave-uniform loop.  (Per prefix and per R: not
//                                    the shape of front_rejoin, which is per level.)
//                         The records of a prefix (at most 64, lane R - 1 its own) are front_reserve's: all of them or none.
//
// The record list starts at candidates + 4096 entries; a check that found more has counted them and is repeated once with exactly that
// room (run_counted, scan_tile.hpp: the dense scans' repeat, here around the check; the two searches' host stage is search_stage there).
// The scan is not repeated.  The substitution check (variants_check_kernel rewrites the candidates in place) runs afterwards.
#include "indels.hpp"
#include "front_search.hpp"

namespace jk {

enum { IC_LOOKUPS = 1 };                                                 // control word 1: table lookups made

// A string of up to 192 two-bit codes as two bit planes of three wave-uniform words each: bit i of a plane = that bit of code i.
struct Plane { unsigned long long a, b, c; };
__device__ __forceinline__ Plane pl_shl(Plane t, int L) {      // 1 <= L < 64
    Plane u;
    u.c = (t.c << L) | (t.b >> (64 - L));
    u.b = (t.b << L) | (t.a >> (64 - L));
    u.a = t.a << L;
    return u;
}
__device__ __forceinline__ Plane pl_shr(Plane t, int L) {      // 1 <= L < 64
    Plane u;
    u.a = (t.a >> L) | (t.b << (64 - L));
    u.b = (t.b >> L) | (t.c << (64 - L));
    u.c = t.c >> L;
    return u;
}
// one plane of the virtual strings; t = that plane of the context, m = the low k - 1 bits (F), xbit = that bit of x
__device__ __forceinline__ Plane pl_prefix(Plane t, unsigned long long m, bool xbit) {      // F x x x ..
    Plane u;
    u.a = (t.a & m) | (xbit ? ~m : 0ull);
    u.b = u.c = xbit ? ~0ull : 0ull;
    return u;
}
__device__ __forceinline__ Plane pl_ins(Plane t, unsigned long long m, int k, int L, bool xbit) {      // F + x^L + the context from k - 1 on
    Plane u = t;
    u.a &= ~m;
    u = pl_shl(u, L);
    u.a |= t.a & m;
    if (xbit) {
        const unsigned long long xm = (1ull << L) - 1ull;
        u.a |= xm << (k - 1);
        u.b |= xm >> (64 - (k - 1));                    // (1 <= k - 1 <= 63)
    }
    return u;
}
__device__ __forceinline__ Plane pl_del(Plane t, unsigned long long m, int L) {      // F + the context from k - 1 + L on
    Plane u = pl_shr(t, L);
    u.a = (u.a & ~m) | (t.a & m);
    return u;
}
__device__ __forceinline__ unsigned long long pl_extract(Plane t, int s) {      // bits s .. s + 63, s < 128
    const int o = s & 63;
    const unsigned long long x = s < 64 ? t.a : t.b, y = s < 64 ? t.b : t.c;
    return o ? (x >> o) | (y << (64 - o)) : x;
}
__device__ __forceinline__ unsigned long long id_spread(uint32_t v) {      // bit i -> bit 2i
    unsigned long long x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// the k-mer of the window that starts at code s < 128 of the string (lo, hi): code s + i is bit pair k - 1 - i
__device__ __forceinline__ u128 id_kmer(Plane lo, Plane hi, int s, int k) {
    const unsigned long long r0 = brev64(pl_extract(lo, s)) >> (64 - k), r1 = brev64(pl_extract(hi, s)) >> (64 - k);
    return mk(id_spread((uint32_t)(r0 >> 32)) | (id_spread((uint32_t)(r1 >> 32)) << 1), id_spread((uint32_t)r0) | (id_spread((uint32_t)r1) << 1));
}

__global__ __launch_bounds__(256) void indels_check_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, TableDev R, uint32_t thre, int max_len,
                                                           const Variant *__restrict__ cand, uint64_t ncand, Indel *__restrict__ out, unsigned long long cap,
                                                           unsigned long long *__restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const int k = R.k;
    const int CL = 2 * k - 2 + max_len;                 // context bytes: at most 142
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    unsigned long long nlook = 0;                       // (wave-uniform) lookups of this wave
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ncand; i += nwv) {
        const int64_t p = cand[i].pos;
        const uint32_t seq = cand[i].seq;
        const int x = cand[i].alt & 3;
        const int64_t o0 = offs[seq];
        const int64_t n = offs[seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        if (p < k - 1 || p >= n) continue;              // (wave-uniform; the scan writes no such candidate)
        const int64_t b0 = p - k + 1;
        int c0 = -1, c1 = -1, c2 = -1;                  // codes of context bytes lane, lane + 64, lane + 128
        if (lane < CL && b0 + lane < n) c0 = code(txt[b0 + lane]);
        if (lane + 64 < CL && b0 + lane + 64 < n) c1 = code(txt[b0 + lane + 64]);
        if (lane + 128 < CL && b0 + lane + 128 < n) c2 = code(txt[b0 + lane + 128]);
        const unsigned long long n0 = __ballot(c0 < 0), n1 = __ballot(c1 < 0), n2 = __ballot(c2 < 0);
        const int bases = n0 ? (int)__builtin_ctzll(n0) : n1 ? 64 + (int)__builtin_ctzll(n1) : n2 ? 128 + (int)__builtin_ctzll(n2) : 192;      // ... in a row from byte 0
        const int refc = __shfl(c0, k - 1);
        if (bases < 2 * k - 2 || refc == x) continue;   // no insertion is evaluated, hence no deletion either
        const unsigned long long e0 = __ballot(c0 == x), e1 = __ballot(c1 == x);
        const Plane clo = {__ballot(c0 & 1), __ballot(c1 & 1), __ballot(c2 & 1)}, chi = {__ballot(c0 & 2), __ballot(c1 & 2), __ballot(c2 & 2)};      // the context
        const unsigned long long fm = (1ull << (k - 1)) - 1ull;      // its first k - 1 codes: F
        uint32_t dels = 0;                              // bit L: del(p, L) is evaluated and s[p + L] == x
        for (int L = 1; L <= max_len; ++L) {
            const int at = k - 1 + L;                   // <= 79
            const bool isx = at < 64 ? (e0 >> at) & 1ull : (e1 >> (at - 64)) & 1ull;
            if (isx && bases >= L + 2 * k - 2) dels |= 1u << L;
        }
        // prefix: windows j < max_len of F + x x x ..
        uint32_t cnt = 0xFFFFFFFFu;
        if (lane < max_len) cnt = canon_count(R, id_kmer(pl_prefix(clo, fm, x & 1), pl_prefix(chi, fm, x & 2), lane, k), k);
        nlook += (unsigned)max_len;
        const unsigned long long fail = __ballot(lane < max_len && cnt < thre);
        const int Lp = fail ? (int)__builtin_ctzll(fail) : max_len;      // ins(.., L) can pass for L <= Lp only
        const uint32_t pm = wave_prefix_min32<16>(cnt);      // lane j < 16: the minimum over windows 0 .. j
        const uint32_t cnt0 = __shfl(cnt, 0);
        uint32_t pass = 0;                              // (wave-uniform) bit L - 1: ins L passed; bit 15 + L: del L passed
        uint32_t my_amin = 0, my_rmin = 0;              // lane b: the minima of hypothesis bit b
        for (int L = 1; L <= Lp; ++L) {
            uint32_t a = 0xFFFFFFFFu;
            if (lane < k - 1) a = canon_count(R, id_kmer(pl_ins(clo, fm, k, L, x & 1), pl_ins(chi, fm, k, L, x & 2), L + lane, k), k);
            nlook += (unsigned)(k - 1);
            a = wave_min32(a);
            const uint32_t pl = __shfl(pm, L - 1);
            a = pl < a ? pl : a;
            if (a >= thre) {
                pass |= 1u << (L - 1);
                if (lane == L - 1) my_amin = a;
            }
        }
        if (cnt0 >= thre) {
            for (int L = 1; L <= max_len; ++L) {
                if (!((dels >> L) & 1u)) continue;
                uint32_t a = 0xFFFFFFFFu;
                if (k > 2) {
                    if (lane < k - 2) a = canon_count(R, id_kmer(pl_del(clo, fm, L), pl_del(chi, fm, L), 1 + lane, k), k);
                    nlook += (unsigned)(k - 2);
                    a = wave_min32(a);
                }
                a = cnt0 < a ? cnt0 : a;
                if (a >= thre) {
                    pass |= 1u << (15 + L);
                    if (lane == 15 + L) my_amin = a;
                }
            }
        }
        if (pass == 0) continue;
        // ref: windows 0 .. jmax of s, once
        const int Ld = (pass >> 16) ? 32 - __clz(pass >> 16) : 0;        // the largest deletion that passed
        const int jmax = Ld ? k + Ld - 2 : k - 2;                         // <= 78
        uint32_t ra = 0xFFFFFFFFu, rb = 0xFFFFFFFFu;                      // windows lane and lane + 64
        if (lane <= jmax) ra = canon_count(R, id_kmer(clo, chi, lane, k), k);
        if (lane + 64 <= jmax) rb = canon_count(R, id_kmer(clo, chi, lane + 64, k), k);
        nlook += (unsigned)(jmax + 1);
        if (pass & 0xFFFFu) {
            const uint32_t r = wave_min32(lane <= k - 2 ? ra : 0xFFFFFFFFu);
            if (lane < 16) my_rmin = r;
        }
        for (int L = 1; L <= Ld; ++L) {
            if (!((pass >> (15 + L)) & 1u)) continue;
            const int lim = k + L - 2;
            uint32_t r = lane <= lim ? ra : 0xFFFFFFFFu;
            r = lane + 64 <= lim && rb < r ? rb : r;
            r = wave_min32(r);
            if (lane == 15 + L) my_rmin = r;
        }
        unsigned long long base = 0;
        const unsigned total = __popc(pass);
        if (lane == 0) base = atomicAdd(&ctl[SC_CURSOR], (unsigned long long)total);
        base = __shfl(base, 0);
        if (base + total > cap) continue;               // (a wave writes all its records or none: the retry has room for every one)
        if (lane < 32 && ((pass >> lane) & 1u)) {
            Indel v;
            v.pos = p;
            v.seq = seq;
            v.ref_min = my_rmin;
            v.alt_min = my_amin;
            v.len = (uint16_t)((lane & 15) + 1);
            v.type = lane < 16 ? IT_INS : IT_DEL;
            v.base = (uint8_t)((0x54474341u >> (8 * x)) & 0xFFu);         // "ACGT"
            v.kind = my_rmin >= thre ? VK_HET : VK_ERROR;
            for (int q = 0; q < 7; ++q) v.pad[q] = 0;
            out[base + __popc(pass & ((1u << lane) - 1u))] = v;
        }
    }
    if (lane == 0 && nlook) atomicAdd(&ctl[IC_LOOKUPS], nlook);
}

// ---- mixed-base insertions ------------------------------------------------------------------------------------------------------------
enum { MC_LOOKUPS = 1, MC_COMPLEX = 2 };                                 // control words 1 and 2: table lookups made; complex sites

__device__ __forceinline__ uint32_t id_squeeze(uint32_t x) {      // bit 2i -> bit i
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
// pl_ins for any string: F + y + the context from k - 1 on; ybit = that plane of y (bit j = base j, L bits)
__device__ __forceinline__ Plane pl_ins_y(Plane t, unsigned long long m, int k, int L, unsigned long long ybit) {
    Plane u = t;
    u.a &= ~m;
    u = pl_shl(u, L);
    u.a |= t.a & m;
    u.a |= ybit << (k - 1);
    u.b |= ybit >> (64 - (k - 1));                      // (1 <= k - 1 <= 63)
    return u;
}

__global__ __launch_bounds__(256) void indels_mixed_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, TableDev R, uint32_t thre, int max_len,
                                                           const Variant *__restrict__ cand, uint64_t ncand, MixedIns *__restrict__ out, unsigned long long cap,
                                                           unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ cplx) {
    __shared__ uint2 s_strip[4][INDEL_FRONT];           // a wave's next frontier: (y, running minimum)
    const int lane = threadIdx.x & 63;
    uint2 *strip = s_strip[threadIdx.x >> 6];
    const int k = R.k;
    const int CL = 2 * k - 2;                           // context bytes: at most 126
    const u128 kmask = maskbits(2 * k);
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    unsigned long long nlook = 0, ncomplex = 0;         // (wave-uniform)
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ncand; i += nwv) {
        const int64_t p = cand[i].pos;
        const uint32_t seq = cand[i].seq;
        const int x = cand[i].alt & 3;
        const int64_t o0 = offs[seq];
        const int64_t n = offs[seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        if (p < k - 1 || p >= n) continue;              // (wave-uniform; the scan writes no such candidate)
        const int64_t b0 = p - k + 1;
        int c0 = -1, c1 = -1;                           // codes of context bytes lane and lane + 64
        if (lane < CL && b0 + lane < n) c0 = code(txt[b0 + lane]);
        if (lane + 64 < CL && b0 + lane + 64 < n) c1 = code(txt[b0 + lane + 64]);
        const unsigned long long n0 = __ballot(c0 < 0), n1 = __ballot(c1 < 0);
        const int bases = n0 ? (int)__builtin_ctzll(n0) : n1 ? 64 + (int)__builtin_ctzll(n1) : 128;
        const int refc = __shfl(c0, k - 1);
        if (bases < CL || refc == x) continue;          // not evaluated
        const Plane clo = {__ballot(c0 > 0 && (c0 & 1)), __ballot(c1 > 0 && (c1 & 1)), 0ull}, chi = {__ballot(c0 > 0 && (c0 & 2)), __ballot(c1 > 0 && (c1 & 2)), 0ull};
        const unsigned long long fm = (1ull << (k - 1)) - 1ull;
        const u128 F = shr(id_kmer(clo, chi, 0, k), 2); // the k - 1 bases before p
        // level 1: S_1 = {x}
        uint32_t yk = (uint32_t)x, mn = 0xFFFFFFFFu;    // lane i < nf: prefix i, first base in the highest pair, and the minimum over its windows
        int nf = 1;
        if (lane == 0) mn = canon_count(R, band(bor(shl(F, 2), mk(0, (uint64_t)x)), kmask), k);
        nlook += 1;
        if ((uint32_t)__shfl(mn, 0) < thre) continue;
        bool have_ref = false;
        uint32_t rmin = 0;
        for (int t = 1;; ++t) {
            // rejoin: window t, lane i for prefix i
            const uint32_t xt = (0x55555555u * (uint32_t)x) & (t == 16 ? 0xFFFFFFFFu : (1u << (2 * t)) - 1u);
            const bool act = lane < nf && yk != xt;
            const unsigned long long actm = __ballot(act);
            uint32_t a = 0xFFFFFFFFu;
            if (act) {
                const u128 w = band(bor(shl(F, 2 * t), mk(0, yk)), kmask);      // the last k bases of F + y
                a = canon_count(R, band(bor(shl(w, 2), mk(0, (uint64_t)refc)), kmask), k);
            }
            nlook += (unsigned)__popcll(actm);
            a = min32(a, mn);
            uint32_t my_amin;
            const unsigned long long recm = front_rejoin(R, thre, __ballot(act && a >= thre), a, nlook, my_amin, [&](int j) {      // windows t+1 .. k+t-2 of the planes with y put in
                const uint32_t yj = (uint32_t)__builtin_amdgcn_readlane((int)yk, j);
                const unsigned long long rv = brev64((unsigned long long)yj) >> (64 - 2 * t);      // base b: its high bit at 2b, its low bit at 2b + 1
                const unsigned long long yhi = id_squeeze((uint32_t)rv), ylo = id_squeeze((uint32_t)(rv >> 1));
                return id_kmer(pl_ins_y(clo, fm, k, t, ylo), pl_ins_y(chi, fm, k, t, yhi), t + 1 + lane, k);
            });
            if (recm) {
                if (!have_ref) {                        // windows 0 .. k-2 of s, once
                    uint32_t r = 0xFFFFFFFFu;
                    if (lane < k - 1) r = canon_count(R, id_kmer(clo, chi, lane, k), k);
                    nlook += (unsigned)(k - 1);
                    rmin = wave_min32(r);
                    have_ref = true;
                }
                const unsigned long long at = front_reserve(recm, &ctl[SC_CURSOR], cap);
                if (at != FRONT_NONE) {
                    MixedIns v;
                    v.pos = p;
                    v.seq = seq;
                    v.ref_min = rmin;
                    v.alt_min = my_amin;
                    v.bases = (uint32_t)(revpairs64((uint64_t)yk) >> (64 - 2 * t));      // base i in bits 2i, 2i + 1
                    v.len = (uint16_t)t;
                    v.kind = rmin >= thre ? VK_HET : VK_ERROR;
                    for (int q = 0; q < 5; ++q) v.pad[q] = 0;
                    out[at] = v;
                }
            }
            if (t >= max_len) break;
            // extend: the last k bases of F + y + z
            const int tot = front_extend(
                R, thre, yk, mn, nf, INDEL_FRONT,
                [=](int, uint32_t parent) {
                    const uint32_t ny = (parent << 2) | (uint32_t)(lane & 3);
                    return FrontChild<uint32_t>{ny, band(bor(shl(F, 2 * (t + 1)), mk(0, ny)), kmask), true, true};
                },
                [&](int at, int, uint32_t ny, uint32_t m) { strip[at] = make_uint2(ny, m); });
            nlook += 4u * (unsigned)nf;
            if (tot > INDEL_FRONT) {                    // complex: nothing of length > t is reported here
                ++ncomplex;
                if (lane == 0) atomicAdd(&cplx[seq], 1ull);
                break;
            }
            if (tot == 0) break;
            front_handover(tot, [&](int l) {
                const uint2 v = strip[l];
                yk = v.x;
                mn = v.y;
            });
            nf = tot;
        }
    }
    if (lane == 0 && nlook) atomicAdd(&ctl[MC_LOOKUPS], nlook);
    if (lane == 0 && ncomplex) atomicAdd(&ctl[MC_COMPLEX], ncomplex);
}

// ---- het clusters ----------------------------------------------------------------------------------------------------------------------
enum { HC_LOOKUPS = 1, HC_COMPLEX = 2, HC_SEARCHED = 3 };                // control words 1 .. 3: table lookups made; complex and searched candidates

__global__ __launch_bounds__(256) void het_cluster_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, TableDev R, uint32_t thre, int N,
                                                          const Variant *__restrict__ cand, uint64_t ncand, HetCluster *__restrict__ out, unsigned long long cap,
                                                          unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ per) {
    __shared__ ulonglong2 s_y[4][INDEL_FRONT];          // a wave's next frontier: y (.x low, .y high) ...
    __shared__ uint32_t s_mn[4][INDEL_FRONT];           // ... and its running minimum
    const int lane = threadIdx.x & 63;
    ulonglong2 *strip_y = s_y[threadIdx.x >> 6];
    uint32_t *strip_mn = s_mn[threadIdx.x >> 6];
    const int k = R.k;
    const int CL = 2 * k - 2 + N;                       // context bytes: at most 190
    const u128 kmask = maskbits(2 * k), fmask = maskbits(2 * (k - 1));
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    unsigned long long nlook = 0, ncomplex = 0, nsearched = 0;      // (wave-uniform)
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ncand; i += nwv) {
        const int64_t p = cand[i].pos;
        const uint32_t seq = cand[i].seq;
        const int x = cand[i].alt & 3;
        const int64_t o0 = offs[seq];
        const int64_t n = offs[seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        if (p < k - 1 || p >= n) continue;              // (wave-uniform; the scan writes no such candidate)
        const int64_t b0 = p - k + 1;
        int c0 = -1, c1 = -1, c2 = -1;                  // codes of context bytes lane, lane + 64, lane + 128
        if (lane < CL && b0 + lane < n) c0 = code(txt[b0 + lane]);
        if (lane + 64 < CL && b0 + lane + 64 < n) c1 = code(txt[b0 + lane + 64]);
        if (lane + 128 < CL && b0 + lane + 128 < n) c2 = code(txt[b0 + lane + 128]);
        const unsigned long long n0 = __ballot(c0 < 0), n1 = __ballot(c1 < 0), n2 = __ballot(c2 < 0);
        const int bases = n0 ? (int)__builtin_ctzll(n0) : n1 ? 64 + (int)__builtin_ctzll(n1) : n2 ? 128 + (int)__builtin_ctzll(n2) : 192;      // ... in a row from byte 0
        const int refc = __shfl(c0, k - 1);
        if (bases < 2 * k - 1 || refc == x) continue;   // repl(p, 1, ..) is not evaluated, hence none is
        const int Rev = bases - (2 * k - 2) < N ? bases - (2 * k - 2) : N;      // the R that are evaluated: 1 .. Rev
        const Plane clo = {__ballot(c0 > 0 && (c0 & 1)), __ballot(c1 > 0 && (c1 & 1)), __ballot(c2 > 0 && (c2 & 1))},
                    chi = {__ballot(c0 > 0 && (c0 & 2)), __ballot(c1 > 0 && (c1 & 2)), __ballot(c2 > 0 && (c2 & 2))};
        // ref: windows 0 .. k+Rev-2 of s, lane j and, past 64, lane j - 64
        const int jmax = k + Rev - 2;                   // <= 126
        uint32_t ra = 0xFFFFFFFFu, rb = 0xFFFFFFFFu;
        if (lane <= jmax) ra = canon_count(R, id_kmer(clo, chi, lane, k), k);
        nlook += (unsigned)(jmax < 63 ? jmax + 1 : 64);
        const uint32_t pma = wave_prefix_min32<64>(ra);
        if ((uint32_t)__shfl(pma, k - 1) < thre) continue;      // R_max = 0: the sequence's own k-mers are unreliable here
        if (jmax >= 64) {
            if (lane + 64 <= jmax) rb = canon_count(R, id_kmer(clo, chi, lane + 64, k), k);
            nlook += (unsigned)(jmax - 63);
        }
        const uint32_t pmb = min32(wave_prefix_min32<64>(rb), (uint32_t)__shfl(pma, 63));
        const int ri = lane + k - 1;                    // lane R - 1: ref_min(R) is the prefix minimum at window k + R - 2
        const uint32_t va = (uint32_t)__shfl(pma, ri & 63), vb = (uint32_t)__shfl(pmb, ri & 63);
        const uint32_t rmin = ri < 64 ? va : vb;
        const unsigned long long okR = __ballot(lane < Rev && rmin >= thre);
        const int Rmax = ~okR ? (int)__builtin_ctzll(~okR) : 64;      // (>= 1: window k - 1 passed)
        ++nsearched;
        if (lane == 0) atomicAdd(&per[2 * (size_t)seq], 1ull);
        // lane R - 1 < Rmax: the k - 1 bases before p + R, and the k - 1 bases from p + R on
        u128 CW = mk(0, 0), G = mk(0, 0);
        if (lane < Rmax) {
            CW = shr(id_kmer(clo, chi, lane + 1, k), 2);
            G = shr(id_kmer(clo, chi, lane + k, k), 2);
        }
        const unsigned nb = (unsigned)shr(G, 2 * (k - 2)).lo & 3u, lastref = (unsigned)CW.lo & 3u;      // s[p + R] and s[p + R - 1]
        const u128 F = shr(id_kmer(clo, chi, 0, k), 2); // the k - 1 bases before p
        // level 1: S_1 = {x}
        u128 y = mk(0, (uint64_t)x);                    // lane i < nf: prefix i, first base in the highest pair ...
        uint32_t mn = 0xFFFFFFFFu;                      // ... and the minimum over its windows
        int nf = 1;
        if (lane == 0) mn = canon_count(R, band(bor(shl(F, 2), y), kmask), k);
        nlook += 1;
        if ((uint32_t)__shfl(mn, 0) < thre) continue;
        for (int t = 1; t <= N; ++t) {
            const u128 W = t >= k - 1 ? band(y, fmask) : band(bor(shl(F, 2 * t), y), fmask);      // the last k - 1 bases of F + y
            // closure: a prefix that has been back on the sequence for k - 1 bases is not extended
            unsigned long long closedm = 0;             // (wave-uniform) bit i: prefix i is closed
            for (int i2 = 0; i2 < nf; ++i2) {
                const u128 Wi = readlane128(W, i2);
                if (__ballot(lane < Rmax && eq(Wi, CW))) closedm |= 1ull << i2;
            }
            // extend: sixteen prefixes a round, (prefix, z) on lane 4 * prefix + z; lane i keeps the solid mask of prefix i
            const u128 Fs = t + 1 < k ? shl(F, 2 * (t + 1)) : mk(0, 0);      // from t + 1 >= k on the newest window is yz's alone
            unsigned solid = 0;
            const int tot = front_extend(
                R, thre, y, mn, nf, INDEL_FRONT,
                [=](int src, u128 parent) {
                    const u128 ny = bor(shl(parent, 2), mk(0, (uint64_t)(lane & 3)));      // (at t = 64 the first base is lost: no child then)
                    return FrontChild<u128>{ny, band(bor(Fs, ny), kmask), true, t < N && !((closedm >> src) & 1ull)};
                },
                [&](int at, int, u128 ny, uint32_t m) {
                    strip_y[at] = make_ulonglong2(ny.lo, ny.hi);
                    strip_mn[at] = m;
                },
                [&](int r0, unsigned long long B) {
                    if (lane >= r0 && lane < r0 + 16) solid = (unsigned)(B >> (4 * (lane - r0))) & 15u;
                });
            nlook += 4u * (unsigned)nf;
            // rejoin: the records of level t, prefix by prefix, lane R - 1 for its own R
            for (int i2 = 0; i2 < nf; ++i2) {
                const u128 yi = readlane128(y, i2), Wi = readlane128(W, i2);
                const unsigned sol = (unsigned)__builtin_amdgcn_readlane((int)solid, i2);
                const uint32_t mni = (uint32_t)__builtin_amdgcn_readlane((int)mn, i2);
                bool alive = lane < Rmax && ((sol >> nb) & 1u) && ((unsigned)yi.lo & 3u) != lastref && !(t == 1 && lane == 0);
                unsigned long long am = __ballot(alive);
                for (int j = 1; j <= 3 && j <= k - 2 && am; ++j) {      // windows t + 1 .. t + 3, each lane its own
                    if (alive) alive = canon_count(R, band(bor(shl(Wi, 2 * (j + 1)), shr(G, 2 * (k - 2 - j))), kmask), k) >= thre;
                    nlook += (unsigned)__popcll(am);
                    am = __ballot(alive);
                }
                unsigned long long recm = 0;            // (wave-uniform) bit R - 1: (R, prefix i2) is a record
                uint32_t my_amin = 0;
                for (unsigned long long q = am; q; q &= q - 1ull) {
                    const int r = (int)__builtin_ctzll(q);
                    const u128 Gr = readlane128(G, r);
                    uint32_t b = 0xFFFFFFFFu;
                    if (lane < k - 1)                   // window t + lane: the last k - 1 - lane bases of W, then lane + 1 bases of G
                        b = canon_count(R, band(bor(shl(Wi, 2 * (lane + 1)), shr(Gr, 2 * (k - 2 - lane))), kmask), k);
                    nlook += (unsigned)(k - 1);
                    b = min32(wave_min32(b), mni);
                    if (b >= thre) {
                        recm |= 1ull << r;
                        if (lane == r) my_amin = b;
                    }
                }
                if (recm) {
                    const unsigned long long at = front_reserve(recm, &ctl[SC_CURSOR], cap);      // (a prefix writes all its records or none)
                    if (at != FRONT_NONE) {
                        const u128 rv = shr(mk(revpairs64(yi.lo), revpairs64(yi.hi)), 128 - 2 * t);      // base i in bits 2i, 2i + 1
                        HetCluster v;
                        v.pos = p;
                        v.seq = seq;
                        v.ref_min = rmin;
                        v.alt_min = my_amin;
                        v.ref_len = (uint32_t)(lane + 1);
                        v.bases[0] = rv.lo;
                        v.bases[1] = rv.hi;
                        v.len = (uint16_t)t;
                        for (int z = 0; z < 6; ++z) v.pad[z] = 0;
                        out[at] = v;
                    }
                }
            }
            if (tot > INDEL_FRONT) {                    // complex: nothing of length > t is listed here
                ++ncomplex;
                if (lane == 0) atomicAdd(&per[2 * (size_t)seq + 1], 1ull);
                break;
            }
            if (tot == 0) break;                        // (also t == N: no child is placed then)
            front_handover(tot, [&](int l) {
                const ulonglong2 v = strip_y[l];
                y = mk(v.y, v.x);
                mn = strip_mn[l];
            });
            nf = tot;
        }
    }
    if (lane == 0 && nlook) atomicAdd(&ctl[HC_LOOKUPS], nlook);
    if (lane == 0 && ncomplex) atomicAdd(&ctl[HC_COMPLEX], ncomplex);
    if (lane == 0 && nsearched) atomicAdd(&ctl[HC_SEARCHED], nsearched);
}

static int indel_check_args(const Table &T, uint32_t thre, int max_len, int cluster_len, std::string &err) {
    if (thre < 1) { err = "indel scan: the threshold (thre) must be at least 1"; return -1; }
    if (T.k < 2) { err = "indel scan: k must be at least 2"; return -1; }
    if (max_len < 1 || max_len > INDEL_MAX_LEN) { err = "indel scan: max_len must be in 1..16"; return -1; }
    if (cluster_len < 0 || cluster_len > CLUSTER_MAX_LEN) { err = "indel scan: cluster_len must be in 1..64"; return -1; }
    return 0;
}

int indel_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, bool mixed, int cluster_len, IndelOut &out,
                      std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "indel scan: bad arguments"; return -1; }
    if (indel_check_args(T, thre, max_len, cluster_len, err)) return -1;
    HIPCHK(hipSetDevice(T.device));
    if (T.materialize(err)) return -1;       // a logically empty table holds garbage until it is zeroed
    out = IndelOut();
    out.counts.assign((size_t)n_seqs * 4, 0);
    out.var.counts.assign((size_t)n_seqs * 3, 0);
    out.mixed = mixed;
    if (mixed) out.mixed_counts.assign((size_t)n_seqs * 3, 0);
    out.cluster_len = cluster_len;
    if (cluster_len) out.cluster_counts.assign((size_t)n_seqs * 4, 0);
    VariantStage S;
    if (variant_scan_stage(T, n_seqs, d_text, offsets, thre, "indel scan", out.var, S, err)) return -1;
    if (S.ntiles == 0) return 0;
    hipStream_t st = T.stream;
    const uint64_t ncand = S.ncand;
    if (ncand) {
        const int W = Table::WS_INDELS;
        unsigned long long *d_ctl = (unsigned long long *)T.workspace(W + 2, SC_WORDS * sizeof(unsigned long long), err), ctl[SC_WORDS] = {0, 0, 0, 0};
        if (!d_ctl) return -1;
        Indel *d_rec = nullptr;
        auto check = [&](unsigned long long cap) {
            d_rec = (Indel *)T.workspace(W + 1, cap * sizeof(Indel), err);
            if (!d_rec) return -1;
            hipLaunchKernelGGL(indels_check_kernel, dim3((unsigned)std::min<uint64_t>((ncand + 3) / 4, 256 * 16)), dim3(256), 0, st, d_text, S.d_offs, T.d, thre, max_len,
                               S.d_cand, ncand, d_rec, cap, d_ctl);
            return 0;
        };
        if (run_counted(st, d_ctl, SC_WORDS, d_ctl, ncand + 4096, "indel scan: the number of records changed between two checks", ctl, out.check_seconds, out.retried, err, check))
            return -1;
        out.lookups = ctl[IC_LOOKUPS];
        out.recs.resize(ctl[SC_CURSOR]);
        if (!out.recs.empty()) HIPCHK(hipMemcpyAsync(out.recs.data(), d_rec, out.recs.size() * sizeof(Indel), hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
    }
    const unsigned search_grid = (unsigned)std::min<uint64_t>((ncand + 3) / 4, 256 * 16);
    if (ncand && mixed) {
        const int W = Table::WS_MIXED;
        unsigned long long ctl[SC_WORDS] = {0, 0, 0, 0};
        std::vector<unsigned long long> cplx;           // after the control words: the complex sites per sequence
        const int sums[1] = {MC_COMPLEX};
        if (search_stage(T, W + 1, n_seqs, 1, sums, ncand + 4096, "indel scan: the number of mixed insertions changed between two searches",
                         "indel scan: the complex sites per sequence do not add up", ctl, out.mixed_recs, cplx, out.mixed_seconds, out.mixed_retried, err,
                         [&](unsigned long long cap, unsigned long long *d_ctl, unsigned long long *d_per) {
                             MixedIns *d_rec = (MixedIns *)T.workspace(W, cap * sizeof(MixedIns), err);
                             if (d_rec)
                                 hipLaunchKernelGGL(indels_mixed_kernel, dim3(search_grid), dim3(256), 0, st, d_text, S.d_offs, T.d, thre, max_len, S.d_cand, ncand, d_rec, cap,
                                                    d_ctl, d_per);
                             return d_rec;
                         }))
            return -1;
        out.mixed_lookups = ctl[MC_LOOKUPS];
        for (size_t i = 0; i < cplx.size(); ++i) out.mixed_counts[3 * i + 2] = cplx[i];
    }
    if (ncand && cluster_len) {
        const int W = Table::WS_CLUSTERS;
        unsigned long long ctl[SC_WORDS] = {0, 0, 0, 0};
        std::vector<unsigned long long> per;            // after the control words: per sequence the searched and the complex candidates
        const int sums[2] = {HC_SEARCHED, HC_COMPLEX};
        if (search_stage(T, W + 1, n_seqs, 2, sums, ncand + 4096, "indel scan: the number of het clusters changed between two searches",
                         "indel scan: the searched and complex candidates per sequence do not add up", ctl, out.cluster_recs, per, out.cluster_seconds, out.cluster_retried, err,
                         [&](unsigned long long cap, unsigned long long *d_ctl, unsigned long long *d_per) {
                             HetCluster *d_rec = (HetCluster *)T.workspace(W, cap * sizeof(HetCluster), err);
                             if (d_rec)
                                 hipLaunchKernelGGL(het_cluster_kernel, dim3(search_grid), dim3(256), 0, st, d_text, S.d_offs, T.d, thre, cluster_len, S.d_cand, ncand, d_rec,
                                                    cap, d_ctl, d_per);
                             return d_rec;
                         }))
            return -1;
        out.cluster_lookups = ctl[HC_LOOKUPS];
        for (size_t i = 0; i < (size_t)n_seqs; ++i) {
            out.cluster_counts[4 * i] = per[2 * i];
            out.cluster_counts[4 * i + 3] = per[2 * i + 1];
        }
        if (het_cluster_finish(out.cluster_recs, n_seqs, cluster_len, out.cluster_counts, err)) return -1;
    }
    if (variant_check_stage(T, n_seqs, d_text, thre, "indel scan", S, out.var, err)) return -1;
    out.seconds = out.var.seconds + out.check_seconds + out.mixed_seconds + out.cluster_seconds;
    std::sort(out.recs.begin(), out.recs.end(), [](const Indel &a, const Indel &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.pos != b.pos ? a.pos < b.pos : a.type != b.type ? a.type < b.type : a.len != b.len ? a.len < b.len : a.base < b.base;
    });
    for (const Indel &v : out.recs) {
        if (v.seq >= (uint32_t)n_seqs || (v.type != IT_INS && v.type != IT_DEL) || (v.kind != VK_HET && v.kind != VK_ERROR)) {
            err = "indel scan: a record the check cannot have written";
            return -1;
        }
        ++out.counts[4 * (size_t)v.seq + 2 * (v.type - 1) + (v.kind - 1)];
    }
    auto korder = [](const MixedIns &v) {               // y with its first base in the highest pair: numeric order is lexicographic order
        uint32_t r = 0;
        for (int i = 0; i < (int)v.len; ++i) r = (r << 2) | ((v.bases >> (2 * i)) & 3u);
        return r;
    };
    for (const MixedIns &v : out.mixed_recs) {
        if (v.seq >= (uint32_t)n_seqs || v.pos < 0 || (v.kind != VK_HET && v.kind != VK_ERROR) || v.len < 1 || (int)v.len > max_len ||
            (v.len < 16 && (v.bases >> (2 * v.len)) != 0u)) {
            err = "indel scan: a mixed insertion the search cannot have written";
            return -1;
        }
        ++out.mixed_counts[3 * (size_t)v.seq + (v.kind - 1)];
    }
    std::sort(out.mixed_recs.begin(), out.mixed_recs.end(), [&](const MixedIns &a, const MixedIns &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.pos != b.pos ? a.pos < b.pos : a.len != b.len ? a.len < b.len : korder(a) < korder(b);
    });
    return 0;
}

int indel_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, bool mixed, int cluster_len, IndelOut &out,
                    std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "indel scan: bad arguments"; return -1; }
    if (indel_check_args(T, thre, max_len, cluster_len, err)) return -1;
    HostText H;
    if (pack_host_text(T, Table::WS_INDELS, n_seqs, seqs, lens, "indel scan", H, err)) return -1;
    return indel_scan_device(T, n_seqs, H.d_text, H.offs.data(), thre, max_len, mixed, cluster_len, out, err);
}

}  // namespace jk
