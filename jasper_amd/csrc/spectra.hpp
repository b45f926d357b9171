// spectra.hpp -- copy-number k-mer spectrum: the join of two resident tables (reads R, assembly A) on the device (spectra.hip), and what
// a slot sweep of this kind is made of, shared with the join of three tables (diploid.hip): the batch load, the flush and the grid.
//
// An extension: the reference has no counterpart.  Semantics: include/jasper_hip.h (jasper_table_spectrum).
#pragma once
#include "table.hpp"
#include <algorithm>
#include <string>

namespace jk {

constexpr int SP_ROWS = 6;          // copies in the assembly: 0, 1, 2, 3, 4, 5 and more
constexpr int SP_COLS = 10002;      // count in the reads, binned as the histogram is: 0 .. 10000, 10001 and more
constexpr int SP_LDS_COLS = 1024;   // columns below it are binned in LDS, the rare tail goes to the global matrix by atomics
constexpr int SP_THREADS = 256, SP_BATCH = 4;   // slots a thread has in flight per trip

// SP_BATCH slots of the swept table per thread and trip: slot, hash and count of those that hold a key, and the home slot of each key
// in the other table O (loads issued together).  `slots` = the swept slot array (S.slots, or one shard of an attached S).
struct SpBatch {
    u128 h[SP_BATCH];
    unsigned long long cnt[SP_BATCH];    // count in the swept table (0: no key)
    ulonglong2 ent[SP_BATCH];            // the key's home slot in the other table
};
__device__ __forceinline__ void sp_load(const TableDev &S, const unsigned long long *__restrict__ slots, const TableDev &O, uint64_t base, uint64_t stride,
                                        uint64_t nslots, SpBatch &b) {
    ulonglong2 e[SP_BATCH];
#pragma unroll
    for (int u = 0; u < SP_BATCH; ++u) {
        const uint64_t i = base + (uint64_t)u * stride;
        e[u] = make_ulonglong2(0ull, 0ull);
        if (i < nslots) e[u] = *reinterpret_cast<const ulonglong2 *>(slots + 2 * i);   // tag + count, one 16-B load
    }
#pragma unroll
    for (int u = 0; u < SP_BATCH; ++u) {
        const uint64_t i = base + (uint64_t)u * stride;
        const bool key = e[u].x != 0ull && e[u].y != 0ull;      // (a slot whose count is 0 is no key: histo_kernel's rule)
        b.cnt[u] = key ? e[u].y : 0ull;
        b.h[u] = mk(0, 0);
        b.ent[u] = make_ulonglong2(0ull, 0ull);
        if (key) {
            b.h[u] = slot_hash(S, i, e[u].x);
            b.ent[u] = *reinterpret_cast<const ulonglong2 *>(read_slots(O, b.h[u]) + 2 * home_of(b.h[u], O.B, O.s));
        }
    }
}

// The one flush of a workgroup whose LDS bins are [ROWS][SP_LDS_COLS]: 64-bit global adds of the non-zero bins into out[ROWS][SP_COLS].
// Every thread of the block calls it after the barrier that ends the binning.
template <int ROWS> __device__ __forceinline__ void sp_flush(const unsigned int *bins, unsigned long long *__restrict__ out) {
    for (int i = threadIdx.x; i < ROWS * SP_LDS_COLS; i += SP_THREADS)
        if (bins[i]) atomicAdd(&out[(size_t)(i / SP_LDS_COLS) * SP_COLS + (i % SP_LDS_COLS)], (unsigned long long)bins[i]);
}

// workgroups of a sweep: fills the chip (256 CUs x 8), the rest is grid-stride; a workgroup's 32-bit LDS bins hold what it sweeps
inline unsigned sweep_grid(uint64_t nslots) {
    uint64_t b = (nslots + (uint64_t)SP_THREADS * SP_BATCH - 1) / ((uint64_t)SP_THREADS * SP_BATCH);
    b = std::min<uint64_t>(std::max<uint64_t>(b, 1), 256 * 8);
    while (nslots / b >= 0xFFFFFFFFull) b *= 2;
    return (unsigned)b;
}

// out: SP_ROWS * SP_COLS cells, row-major (host memory); seconds: device time (HIP events) of the sweeps
int table_spectrum(Table &R, Table &A, uint64_t *out, double *seconds, std::string &err);

}  // namespace jk
