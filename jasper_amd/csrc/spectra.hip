// spectra.hip -- copy-number k-mer spectrum and its completeness numbers: two resident tables of one k (reads R, assembly A) joined on
// the device into S[6][10002] (semantics: include/jasper_hip.h, jasper_table_spectrum).
//
// An extension the reference has no counterpart for (the spectra-cn / completeness half of a k-mer evaluation).  A slot stores its key
// as (home, remainder), so slot_hash gives back the key's mixed hash -- a value of 2k bits that does not depend on the table's size --
// and table_get finds it in the other table, narrow or wide.  No key leaves the device.
//
//   spectra_reads_kernel   sweep A, over the slots of R (of one owner's shard when R is attached): slot -> hash -> count in A ->
//                          bin [min(copies, 5)][min(clamp32(count), 10001)].  Columns below SP_LDS_COLS are binned in LDS (6 x 1024 x
//                          4 B = 24 KB), the rare tail beyond goes to the global matrix by 64-bit atomics.
//   spectra_asm_kernel     sweep B, over the slots of A: slot -> hash -> count in R (through read_slots: the owner's shard) -> where R
//                          has none, bin [min(copies, 5)][0].  Five counters per thread, summed per wave, then per workgroup in LDS.
//
// Both take SP_BATCH slots per thread and trip (coalesced 16-B loads) and have the home-slot loads of the other table in flight for all
// of them before any is resolved (table_get_prefetched): a sweep is otherwise one dependent HBM round trip per key.  One flush per
// workgroup: 64-bit global adds of the non-zero bins; integer sums, so the result does not depend on the order.
#include "spectra.hpp"
#include <vector>

namespace jk {

#define HIPCHK(x)                                                                     \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            err = std::string(#x) + ": " + hipGetErrorString(e_);                     \
            return -1;                                                                \
        }                                                                             \
    } while (0)

__global__ __launch_bounds__(SP_THREADS) void spectra_reads_kernel(TableDev R, const unsigned long long *__restrict__ slots, TableDev A,
                                                                   unsigned long long *__restrict__ out) {
    __shared__ unsigned int bins[SP_ROWS * SP_LDS_COLS];
    for (int i = threadIdx.x; i < SP_ROWS * SP_LDS_COLS; i += SP_THREADS) bins[i] = 0;
    __syncthreads();
    const uint64_t nslots = R.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    for (uint64_t base = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; base < nslots; base += stride * SP_BATCH) {
        SpBatch b;
        sp_load(R, slots, A, base, stride, nslots, b);
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            if (b.cnt[u] == 0ull) continue;
            const unsigned long long m = table_get_prefetched(A, b.h[u], b.ent[u]);
            const uint32_t row = m > (unsigned long long)(SP_ROWS - 1) ? (uint32_t)(SP_ROWS - 1) : (uint32_t)m;
            const uint32_t c = clamp32(b.cnt[u]);
            const uint32_t col = c > (uint32_t)(SP_COLS - 1) ? (uint32_t)(SP_COLS - 1) : c;
            if (col < (uint32_t)SP_LDS_COLS) atomicAdd(&bins[row * SP_LDS_COLS + col], 1u);
            else atomicAdd(&out[(size_t)row * SP_COLS + col], 1ull);
        }
    }
    __syncthreads();
    sp_flush<SP_ROWS>(bins, out);
}

__global__ __launch_bounds__(SP_THREADS) void spectra_asm_kernel(TableDev A, TableDev R, unsigned long long *__restrict__ out) {
    __shared__ unsigned int bins[SP_ROWS];
    if (threadIdx.x < SP_ROWS) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t nslots = A.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    uint32_t n1 = 0, n2 = 0, n3 = 0, n4 = 0, n5 = 0;      // assembly-only keys of this thread by copies (named, not indexed: no scratch)
    for (uint64_t base = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; base < nslots; base += stride * SP_BATCH) {
        SpBatch b;
        sp_load(A, A.slots, R, base, stride, nslots, b);
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            if (b.cnt[u] == 0ull) continue;
            if (table_get_prefetched(R, b.h[u], b.ent[u]) != 0ull) continue;
            const unsigned long long m = b.cnt[u];
            n1 += m == 1ull;
            n2 += m == 2ull;
            n3 += m == 3ull;
            n4 += m == 4ull;
            n5 += m >= 5ull;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n1 += __shfl_xor(n1, o);
        n2 += __shfl_xor(n2, o);
        n3 += __shfl_xor(n3, o);
        n4 += __shfl_xor(n4, o);
        n5 += __shfl_xor(n5, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n1) atomicAdd(&bins[1], n1);
        if (n2) atomicAdd(&bins[2], n2);
        if (n3) atomicAdd(&bins[3], n3);
        if (n4) atomicAdd(&bins[4], n4);
        if (n5) atomicAdd(&bins[5], n5);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < SP_ROWS && bins[threadIdx.x]) atomicAdd(&out[(size_t)threadIdx.x * SP_COLS], (unsigned long long)bins[threadIdx.x]);
}

namespace {
struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

int table_spectrum(Table &R, Table &A, uint64_t *out, double *seconds, std::string &err) {
    if (!out) { err = "spectrum: null output"; return -1; }
    if (&R == &A) { err = "spectrum: the read table and the assembly table are the same table"; return -1; }
    if (R.k != A.k) { err = "spectrum: the tables have different k (" + std::to_string(R.k) + " and " + std::to_string(A.k) + ")"; return -1; }
    if (R.device != A.device) { err = "spectrum: the tables are on different devices"; return -1; }
    if (A.d.nshard > 1) { err = "spectrum: the assembly table must be a whole table, not an attached owner-sharded one"; return -1; }
    HIPCHK(hipSetDevice(R.device));
    // a logically empty table holds garbage until it is zeroed: both tables are read slot by slot and probed
    if (A.materialize(err) || R.materialize(err)) return -1;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "spectrum words");
    const size_t bytes = (size_t)SP_ROWS * SP_COLS * sizeof(unsigned long long);
    unsigned long long *d_out = (unsigned long long *)R.workspace(Table::WS_SPECTRA, bytes, err);
    if (!d_out) return -1;
    Events ev;
    for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
    hipStream_t st = R.stream;
    HIPCHK(hipEventRecord(ev.e[0], A.stream));        // whatever A's stream still does to A comes first
    HIPCHK(hipStreamWaitEvent(st, ev.e[0], 0));
    HIPCHK(hipMemsetAsync(d_out, 0, bytes, st));
    HIPCHK(hipEventRecord(ev.e[1], st));
    const uint32_t nsh = R.d.nshard > 1 ? R.d.nshard : 1;
    for (uint32_t s = 0; s < nsh; ++s) {               // every owner's shard has R's geometry (attach checks it)
        const unsigned long long *slots = R.d.nshard > 1 ? R.d.shard[s] : R.d.slots;
        hipLaunchKernelGGL(spectra_reads_kernel, dim3(sweep_grid(R.nslots)), dim3(SP_THREADS), 0, st, R.d, slots, A.d, d_out);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(spectra_asm_kernel, dim3(sweep_grid(A.nslots)), dim3(SP_THREADS), 0, st, A.d, R.d, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[2], st));
    HIPCHK(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
    if (seconds) *seconds = ms * 1e-3;
    return 0;
}

}  // namespace jk
