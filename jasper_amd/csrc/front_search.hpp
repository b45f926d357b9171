// front_search.hpp -- what the four front searches (indels_mixed_kernel and het_cluster_kernel in indels.hip, compound_search_kernel in
// compound.hip, gap_search_kernel in gaps.hip) have in common: a bounded breadth-first search over the strings the reads hold between two
// flanks, one wave per site, the frontier of at most `cap` = 64 strings one per lane.  Device pieces that a kernel calls; how a kernel
// loads its site, what its key is, what it fills into a record and when a site is closed or complex stay the kernel's own.
//
//   front_flanks      F = the k - 1 bases before a and G = the k - 1 bases from q on as two wave-uniform 128-bit words (base l in bit pair
//                     k - 2 - l), or "a flank holds a non-base".
//   front_extend      one level's extend step, sixteen strings a round: (string, z) on lane 4 * string + z.  The ballot of a round is in
//                     (string, z) order -- lane order is the frontier's order -- so a child's place is a popcount; places from `cap` on are
//                     not stored.  Returns the number of children, which the caller compares with `cap`.
//   front_handover    the children through the wave's LDS strip into the lanes that own them from now on, between two wave barriers.
//   front_window0, front_window, front_rejoin   the rejoin: window t of string + G on the string's own lane, then in a wave-uniform loop over
//                     the strings that passed it windows t + 1 .. t + k - 2, lane j window t + 1 + j, one wave minimum each.
//   front_reserve     the records of a level (lane i its own) take one returning cursor add; a level writes all its records or none, in
//                     both lists if it has two.  The cursor has counted them either way (run_counted, scan_tile.hpp).
// Every lane of the wave calls each of them (they hold ballots, shuffles and wave barriers); the lambdas are inlined.
#pragma once
#include "scan_tile.hpp"

namespace jk {

// F and G of the site (a, q) of the sequence txt: both lie inside it (the caller has checked).  bases false: one of them holds a non-base
// (F and G are not made then).
struct Flanks { u128 F, G; bool bases; };
__device__ __forceinline__ Flanks front_flanks(const uint8_t *__restrict__ txt, int64_t a, int64_t q, int k) {
    const int lane = threadIdx.x & 63;
    int cf = 0, cg = 0;
    if (lane < k - 1) {
        cf = code(txt[a - (k - 1) + lane]);
        cg = code(txt[q + lane]);
    }
    if (__ballot(cf < 0 || cg < 0)) return Flanks{mk(0, 0), mk(0, 0), false};
    const unsigned sh = lane < k - 1 ? 2u * (unsigned)(k - 2 - lane) : 0u;
    const u128 f1 = lane < k - 1 ? shl(mk(0, (uint64_t)cf), sh) : mk(0, 0), g1 = lane < k - 1 ? shl(mk(0, (uint64_t)cg), sh) : mk(0, 0);
    return Flanks{mk(readfirstlane64(wave_or64(f1.hi)), readfirstlane64(wave_or64(f1.lo))), mk(readfirstlane64(wave_or64(g1.hi)), readfirstlane64(wave_or64(g1.lo))), true};
}

__device__ __forceinline__ uint32_t front_shfl(uint32_t key, int src) { return (uint32_t)__shfl(key, src); }
__device__ __forceinline__ u128 front_shfl(u128 key, int src) { return mk(__shfl(key.hi, src), __shfl(key.lo, src)); }

// What a kernel says of the child (parent, z = lane & 3) on this lane: its key, the k-mer of its newest window, whether that is looked up at
// all, and whether the child may enter the next frontier if it is solid.
template <class Key> struct FrontChild { Key key; u128 kmer; bool look, enters; };

// Lane i < nf holds string i's key (32 or 128 bits) and running minimum mn.  child(src, parent) -> FrontChild<Key> for the parent on lane
// src < 64 (src >= nf is never looked up); place(at, src, key, m) stores the child at place at < cap of the strip, m = its running minimum;
// seen(r0, B) gets each round's ballot of the solid children, those that may not enter too.
template <class Key, class Child, class Place, class Seen>
__device__ __forceinline__ int front_extend(const TableDev &R, uint32_t thre, Key key, uint32_t mn, int nf, int cap, Child &&child, Place &&place, Seen &&seen) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int tot = 0;
    for (int r0 = 0; r0 < nf; r0 += 16) {
        const int src = r0 + (lane >> 2);               // <= 63
        const FrontChild<Key> C = child(src, front_shfl(key, src));
        const uint32_t pm = (uint32_t)__shfl(mn, src);
        const bool from = src < nf && C.look;
        uint32_t c = 0;
        if (from) c = canon_count(R, C.kmer, R.k);
        const bool ok = from && c >= thre;
        seen(r0, __ballot(ok));
        const bool in = ok && C.enters;
        const unsigned long long B = __ballot(in);
        const int at = tot + __popcll(B & below);
        if (in && at < cap) place(at, src, C.key, min32(pm, c));
        tot += __popcll(B);
    }
    return tot;
}
template <class Key, class Child, class Place>
__device__ __forceinline__ int front_extend(const TableDev &R, uint32_t thre, Key key, uint32_t mn, int nf, int cap, Child &&child, Place &&place) {
    return front_extend(R, thre, key, mn, nf, cap, child, place, [](int, unsigned long long) {});
}

// The strip hand-over after an extend step that left 0 < tot <= cap children: take(lane) runs on the lanes < tot and reads place `lane` of
// the strip (and may store to global memory what later levels read back: the gap search's log row).
// Before it, a release / barrier / acquire of wavefront scope: every lane's stores to the strip are performed before any lane's load from
// it.  After it the same three: every lane's loads from the strip are performed before the next level's stores to it, and what take stored
// is performed before any lane of the wave loads it.  The fences keep the compiler from moving memory operations across; the hardware
// performs one wave's LDS operations, and its vector memory operations to global memory, in the order they were issued.
template <class Take> __device__ __forceinline__ void front_handover(int tot, Take &&take) {
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < tot) take(lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W = the last k - 1 bases of F + (a string), G as front_flanks leaves it.  Window t of string + G, the first that holds a base of G ...
__device__ __forceinline__ u128 front_window0(u128 W, u128 G, int k, u128 kmask) { return band(bor(shl(W, 2), shr(G, 2 * (k - 2))), kmask); }
// ... and window t + 1 + lane, lane < k - 2: the last k - 2 - lane bases of W, then lane + 2 bases of G
__device__ __forceinline__ u128 front_window(u128 W, u128 G, int k, u128 kmask) {
    const int lane = threadIdx.x & 63;
    return band(bor(shl(W, 2 * (lane + 2)), shr(G, 2 * (k - 3 - lane))), kmask);
}

// The rejoin tail.  P (wave-uniform): bit i = string i passed window t; a = on lane i the minimum over string i's windows up to t.
// window(j), j wave-uniform, is this lane's window t + 1 + lane of string j (asked of lanes < k - 2 only).  Returns the mask of the strings
// all of whose windows are solid -- the records of the level -- and leaves the minimum of record i in alt_min on lane i.  k - 2 lookups per
// bit of P are added to nlook.
template <class Window>
__device__ __forceinline__ unsigned long long front_rejoin(const TableDev &R, uint32_t thre, unsigned long long P, uint32_t a, unsigned long long &nlook, uint32_t &alt_min,
                                                           Window &&window) {
    const int lane = threadIdx.x & 63;
    const int k = R.k;
    alt_min = a;
    if (k <= 2) return P;
    unsigned long long recm = 0;
    for (unsigned long long p = P; p; p &= p - 1ull) {
        const int j = (int)__builtin_ctzll(p);
        const uint32_t aj = (uint32_t)__builtin_amdgcn_readlane((int)a, j);
        uint32_t b = 0xFFFFFFFFu;
        if (lane < k - 2) b = canon_count(R, window(j), k);
        nlook += (unsigned)(k - 2);
        b = min32(wave_min32(b), aj);
        if (b >= thre) {
            recm |= 1ull << j;
            if (lane == j) alt_min = b;
        }
    }
    return recm;
}

// Places for the records recm != 0 of a level in a list of cap entries: lane 0 adds their number to *cursor.  Returns this lane's place, or
// FRONT_NONE if the lane has no record or the level does not fit.  With a second list (the gap search's byte pool: each2 entries per
// record, cap2 in all) its cursor is added to right after the first, *at2 is the lane's first entry there, and the level has to fit both.
constexpr unsigned long long FRONT_NONE = ~0ull;
__device__ __forceinline__ unsigned long long front_reserve(unsigned long long recm, unsigned long long *cursor, unsigned long long cap, unsigned long long *cursor2 = nullptr,
                                                            unsigned long long each2 = 0, unsigned long long cap2 = 0, unsigned long long *at2 = nullptr) {
    const int lane = threadIdx.x & 63;
    const unsigned total = __popcll(recm), mine = __popcll(recm & ((1ull << lane) - 1ull));
    unsigned long long base = 0, base2 = 0;
    if (lane == 0) {
        base = atomicAdd(cursor, (unsigned long long)total);
        if (cursor2) base2 = atomicAdd(cursor2, total * each2);
    }
    base = __shfl(base, 0);
    bool fits = base + total <= cap;
    if (cursor2) {
        base2 = __shfl(base2, 0);
        fits = fits && base2 + total * each2 <= cap2;
        *at2 = base2 + mine * each2;
    }
    return fits && ((recm >> lane) & 1ull) ? base + mine : FRONT_NONE;
}

}  // namespace jk
