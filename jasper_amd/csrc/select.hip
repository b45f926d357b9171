// select.hip -- a join of up to three resident tables materialised as a table: the keys of S (`src`) whose count is at least thre_src,
// that A (`absent`) does not hold and that R (`solid`, optional) holds at least thre_solid times, with their counts in S, as the keys
// of a fourth table (semantics: include/jasper_hip.h, jasper_table_select).
//
// An extension the reference has no counterpart for.  The hap-mer census (hapmers.hip) counts such a set; the binning kernels take
// tables, so a set that is a table serves all of them unchanged -- and a set of markers is far smaller than the tables it comes from.
//
//   table_select_kernel   a sweep over the slots [first, end) of S in the shape of hapmer_census_kernel: 16-byte slot loads, slots below
//                         the threshold dropped before any probe, the others probe A with the home-slot loads of the batch in flight
//                         together, the survivors probe R by a plain table_get (through read_slots: the owner's shard when R is
//                         attached).  What survives that is an ENTRY {hash.hi, hash.lo, count in S}, the layout of export_kernel /
//                         import_kernel.  The entries of a wave and trip are ranked by ballot and popcount and placed behind ONE
//                         returning add on the piece's cursor; nothing is written at or beyond `cap` entries.  The loop variable
//                         is the workgroup's, so every lane of a wave makes the same trips and reaches the ballots; the slot bound
//                         is checked per slot inside.  No lane waits for another.  Four counters per thread, summed per wave and per
//                         workgroup, four global adds per workgroup.
// Host side (table_select): the tables ordered by settle as the census orders its own, S walked in pieces of at most SEL_PIECE slots
// (JASPER_SELECT_PIECE=<slots> for tests), the entry buffer one piece's slots long -- a piece cannot overflow it and it does not grow
// with the table -- and each piece's entries given to Table::import_entries of the destination, whose capacity check, spill and
// growth are what every import has.  No insert code here.
//
//   table_subtract_kernel the same sweep for dst = S - M (`minus`): every key of S probes M once, by table_get_prefetched, whose result is
//                         the full 64-bit count; an entry is {hash.hi, hash.lo, count in S - count in M} where that is above 0.  One probe
//                         where the select has two, five counters, the same ballot ranking and the same single add on the cursor.
// Host side (table_subtract): table_select's loop with JASPER_SUBTRACT_PIECE for its piece; both sources are only read.
#include "select.hpp"
#include "scan_tile.hpp"
#include "spectra.hpp"
#include <cstdlib>

namespace jk {

enum { SEL_CTL = 1 + SEL_NCOUNT };                      // control words of a piece: the entry cursor, then the four counters

__global__ __launch_bounds__(SP_THREADS) void table_select_kernel(TableDev S, TableDev A, TableDev R, int has_r, uint64_t first, uint64_t end, uint32_t thre_src,
                                                                  uint32_t thre_solid, unsigned long long *__restrict__ entries, unsigned long long cap,
                                                                  unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_sum[SEL_NCOUNT];
    if (threadIdx.x < SEL_NCOUNT) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;               // the lanes before mine
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    uint32_t nc = 0, na = 0, nn = 0, ns = 0;
    // (blk is the same in every thread of the workgroup: a wave's lanes make the same trips, whatever their slots are)
    for (uint64_t blk = first + blockIdx.x * (uint64_t)SP_THREADS; blk < end; blk += stride * SP_BATCH) {
        const uint64_t base = blk + threadIdx.x;
        ulonglong2 e[SP_BATCH], ent[SP_BATCH];
        u128 h[SP_BATCH];
        bool cand[SP_BATCH], sel[SP_BATCH];
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            e[u] = make_ulonglong2(0ull, 0ull);
            if (i < end) e[u] = *reinterpret_cast<const ulonglong2 *>(S.slots + 2 * i);   // tag + count, one 16-B load
        }
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            cand[u] = e[u].x != 0ull && e[u].y >= (unsigned long long)thre_src;      // (thre_src >= 1: a slot whose count is 0 is no key)
            h[u] = mk(0, 0);
            ent[u] = make_ulonglong2(0ull, 0ull);
            if (cand[u]) {
                h[u] = slot_hash(S, i, e[u].x);
                ent[u] = *reinterpret_cast<const ulonglong2 *>(A.slots + 2 * home_of(h[u], A.B, A.s));
            }
        }
        unsigned long long bal[SP_BATCH];
        uint32_t total = 0;
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            sel[u] = false;
            if (cand[u]) {
                ++nc;
                if (table_get_prefetched(A, h[u], ent[u]) != 0ull) ++na;
                else if (has_r && clamp32(table_get(R, h[u])) < thre_solid) ++nn;
                else sel[u] = true;
            }
            ns += sel[u] ? 1u : 0u;
            bal[u] = __ballot(sel[u]);
            total += (uint32_t)__popcll(bal[u]);
        }
        if (total) {                                    // (the same in every lane of the wave)
            unsigned long long at = 0ull;
            if (lane == 0) at = atomicAdd(&ctl[0], (unsigned long long)total);
            at = readfirstlane64(at);
#pragma unroll
            for (int u = 0; u < SP_BATCH; ++u) {
                const unsigned long long idx = at + (unsigned long long)__popcll(bal[u] & below);
                if (sel[u] && idx < cap) {
                    entries[3 * idx + 0] = h[u].hi;
                    entries[3 * idx + 1] = h[u].lo;
                    entries[3 * idx + 2] = e[u].y;
                }
                at += (unsigned long long)__popcll(bal[u]);
            }
        }
    }
    nc = wave_sum(nc);
    na = wave_sum(na);
    nn = wave_sum(nn);
    ns = wave_sum(ns);
    if (lane == 0) {
        if (nc) atomicAdd(&s_sum[SEL_CANDIDATES], (unsigned long long)nc);
        if (na) atomicAdd(&s_sum[SEL_IN_ABSENT], (unsigned long long)na);
        if (nn) atomicAdd(&s_sum[SEL_NOT_SOLID], (unsigned long long)nn);
        if (ns) atomicAdd(&s_sum[SEL_SELECTED], (unsigned long long)ns);
    }
    __syncthreads();
    if (threadIdx.x < SEL_NCOUNT && s_sum[threadIdx.x]) atomicAdd(&ctl[1 + threadIdx.x], s_sum[threadIdx.x]);
}

enum { SUB_SUM = SUB_NCOUNT, SUB_CTL = 2 + SUB_NCOUNT };      // control words of a piece: the entry cursor, the five counters, the sum of the differences

__global__ __launch_bounds__(SP_THREADS) void table_subtract_kernel(TableDev S, TableDev M, uint64_t first, uint64_t end, unsigned long long *__restrict__ entries,
                                                                    unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_sum[SUB_NCOUNT + 1];
    if (threadIdx.x <= SUB_NCOUNT) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;               // the lanes before mine
    const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
    uint32_t nw = 0, nm = 0, nd = 0, nu = 0, nk = 0;
    unsigned long long sum = 0ull;                     // of my kept differences (mod 2^64, as the table's occurrence counter runs)
    // (blk is the same in every thread of the workgroup: a wave's lanes make the same trips, whatever their slots are)
    for (uint64_t blk = first + blockIdx.x * (uint64_t)SP_THREADS; blk < end; blk += stride * SP_BATCH) {
        const uint64_t base = blk + threadIdx.x;
        ulonglong2 e[SP_BATCH], ent[SP_BATCH];
        u128 h[SP_BATCH];
        bool key[SP_BATCH], keep[SP_BATCH];
        unsigned long long diff[SP_BATCH];
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            e[u] = make_ulonglong2(0ull, 0ull);
            if (i < end) e[u] = *reinterpret_cast<const ulonglong2 *>(S.slots + 2 * i);   // tag + count, one 16-B load
        }
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            const uint64_t i = base + (uint64_t)u * stride;
            key[u] = e[u].x != 0ull && e[u].y != 0ull;      // (a slot whose count is 0 is no key)
            h[u] = mk(0, 0);
            ent[u] = make_ulonglong2(0ull, 0ull);
            if (key[u]) {
                h[u] = slot_hash(S, i, e[u].x);
                ent[u] = *reinterpret_cast<const ulonglong2 *>(M.slots + 2 * home_of(h[u], M.B, M.s));
            }
        }
        unsigned long long bal[SP_BATCH];
        uint32_t total = 0;
#pragma unroll
        for (int u = 0; u < SP_BATCH; ++u) {
            keep[u] = false;
            diff[u] = 0ull;
            if (key[u]) {
                ++nw;
                const unsigned long long cm = table_get_prefetched(M, h[u], ent[u]);      // (64 bits: no clamp)
                if (cm != 0ull) ++nm;
                if (cm > e[u].y) ++nu;
                else if (cm == e[u].y) ++nd;
                else {
                    keep[u] = true;
                    diff[u] = e[u].y - cm;
                    sum += diff[u];
                }
            }
            nk += keep[u] ? 1u : 0u;
            bal[u] = __ballot(keep[u]);
            total += (uint32_t)__popcll(bal[u]);
        }
        if (total) {                                    // (the same in every lane of the wave)
            unsigned long long at = 0ull;
            if (lane == 0) at = atomicAdd(&ctl[0], (unsigned long long)total);
            at = readfirstlane64(at);
#pragma unroll
            for (int u = 0; u < SP_BATCH; ++u) {
                const unsigned long long idx = at + (unsigned long long)__popcll(bal[u] & below);
                if (keep[u] && idx < cap) {
                    entries[3 * idx + 0] = h[u].hi;
                    entries[3 * idx + 1] = h[u].lo;
                    entries[3 * idx + 2] = diff[u];
                }
                at += (unsigned long long)__popcll(bal[u]);
            }
        }
    }
    nw = wave_sum(nw);
    nm = wave_sum(nm);
    nd = wave_sum(nd);
    nu = wave_sum(nu);
    nk = wave_sum(nk);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if (lane == 0) {
        if (sum) atomicAdd(&s_sum[SUB_SUM], sum);
        if (nw) atomicAdd(&s_sum[SUB_SWEPT], (unsigned long long)nw);
        if (nm) atomicAdd(&s_sum[SUB_MATCHED], (unsigned long long)nm);
        if (nd) atomicAdd(&s_sum[SUB_DROPPED], (unsigned long long)nd);
        if (nu) atomicAdd(&s_sum[SUB_UNDERFLOW], (unsigned long long)nu);
        if (nk) atomicAdd(&s_sum[SUB_KEPT], (unsigned long long)nk);
    }
    __syncthreads();
    if (threadIdx.x <= SUB_NCOUNT && s_sum[threadIdx.x]) atomicAdd(&ctl[1 + threadIdx.x], s_sum[threadIdx.x]);
}

namespace {
// check_trio's checks in its wording, for the four tables of a select
int check_select(Table &dst, Table &src, Table &absent, Table *solid, uint32_t thre_src, uint32_t thre_solid, std::string &err) {
    const std::string w("select");
    Table *all[4] = {&src, &absent, solid, &dst};
    const char *names[4] = {"source", "absent", "solid", "destination"};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (all[i] && all[i] == all[j]) { err = w + ": the " + names[i] + " table and the " + names[j] + " table are the same table"; return -1; }
    for (int i = 1; i < 4; ++i) {
        if (!all[i]) continue;
        if (all[i]->k != src.k) {
            err = w + ": the tables have different k (" + names[0] + " " + std::to_string(src.k) + ", " + names[i] + " " + std::to_string(all[i]->k) + ")";
            return -1;
        }
        if (all[i]->device != src.device) { err = w + ": the tables are on different devices"; return -1; }
    }
    for (int i = 0; i < 4; ++i)
        if (i != 2 && all[i]->d.nshard > 1) { err = w + ": the " + names[i] + " table must be a whole table, not an attached owner-sharded one"; return -1; }
    if (thre_src < 1) { err = w + ": the source threshold must be at least 1 (it is 0)"; return -1; }
    if (thre_solid < 1) { err = w + ": the solid threshold must be at least 1 (it is 0)"; return -1; }
    return 0;
}
unsigned select_grid(uint64_t nslots) {                // as the census's sweeps: fills the chip, the rest is grid-stride
    uint64_t b = (nslots + (uint64_t)SP_THREADS * SP_BATCH - 1) / ((uint64_t)SP_THREADS * SP_BATCH);
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), 256 * 8);
}
int piece_slots(const char *what, const char *name, uint64_t &piece, std::string &err) {
    piece = SEL_PIECE;
    const char *v = getenv(name);
    if (!v) return 0;
    char *rest = nullptr;
    const unsigned long long n = strtoull(v, &rest, 10);
    if (!*v || *rest || n < 1 || n > SEL_PIECE) { err = std::string(what) + ": " + name + " must be a number of slots from 1 to " + std::to_string(SEL_PIECE); return -1; }
    piece = n;
    return 0;
}
// check_select's checks for the three tables of a subtract
int check_subtract(Table &dst, Table &src, Table &minus, std::string &err) {
    const std::string w("subtract");
    Table *all[3] = {&src, &minus, &dst};
    const char *names[3] = {"source", "minus", "destination"};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (all[i] == all[j]) { err = w + ": the " + names[i] + " table and the " + names[j] + " table are the same table"; return -1; }
    for (int i = 1; i < 3; ++i) {
        if (all[i]->k != src.k) {
            err = w + ": the tables have different k (" + names[0] + " " + std::to_string(src.k) + ", " + names[i] + " " + std::to_string(all[i]->k) + ")";
            return -1;
        }
        if (all[i]->device != src.device) { err = w + ": the tables are on different devices"; return -1; }
    }
    for (int i = 0; i < 3; ++i)
        if (all[i]->d.nshard > 1) { err = w + ": the " + names[i] + " table must be a whole table, not an attached owner-sharded one"; return -1; }
    return 0;
}
}  // namespace

int table_select(Table &dst, Table &src, Table &absent, Table *solid, uint32_t thre_src, uint32_t thre_solid, uint64_t out4[4], double *seconds, std::string &err) {
    if (!out4) { err = "select: null output"; return -1; }
    if (check_select(dst, src, absent, solid, thre_src, thre_solid, err)) return -1;
    uint64_t piece = 0;
    if (piece_slots("select", "JASPER_SELECT_PIECE", piece, err)) return -1;
    HIPCHK(hipSetDevice(src.device));
    if (dst.materialize(err) || dst.read_stats(err)) return -1;
    if (dst.h_stats[ST_DISTINCT] != 0) { err = "select: the destination table must be empty (it holds " + std::to_string(dst.h_stats[ST_DISTINCT]) + " keys)"; return -1; }
    Table *others[3] = {&absent, solid, &dst};
    Events order;
    if (settle(src, others, 3, order, err)) return -1;
    hipStream_t st = src.stream;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "select words");
    const uint64_t cap = std::min<uint64_t>(piece, src.nslots);
    unsigned long long *d_ent = (unsigned long long *)src.workspace(Table::WS_SELECT, (size_t)cap * 3 * sizeof(unsigned long long), err);
    if (!d_ent) return -1;
    unsigned long long *d_ctl = (unsigned long long *)src.workspace(Table::WS_SELECT + 1, SEL_CTL * sizeof(unsigned long long), err);
    if (!d_ctl) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    const TableDev rd = solid ? solid->d : src.d;
    double s = 0;
    for (int i = 0; i < SEL_NCOUNT; ++i) out4[i] = 0;
    for (uint64_t first = 0; first < src.nslots; first += piece) {
        const uint64_t end = std::min<uint64_t>(first + piece, src.nslots);
        HIPCHK(hipMemsetAsync(d_ctl, 0, SEL_CTL * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(table_select_kernel, dim3(select_grid(end - first)), dim3(SP_THREADS), 0, st, src.d, absent.d, rd, solid ? 1 : 0, first, end, thre_src, thre_solid,
                           d_ent, (unsigned long long)cap, d_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        unsigned long long res[SEL_CTL];
        HIPCHK(hipMemcpyAsync(res, d_ctl, sizeof res, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        if (ev.add_seconds(s, err)) return -1;
        if (res[0] != res[1 + SEL_SELECTED] || res[0] > end - first) { err = "select: a piece's entry count does not match its counters"; return -1; }
        for (int i = 0; i < SEL_NCOUNT; ++i) out4[i] += res[1 + i];
        // (the kernel has finished: the destination's stream may read the entries, and has read them when import_entries returns)
        if (res[0]) {
            const int rc = dst.import_entries(d_ent, res[0], err);
            if (rc) return rc;
            HIPCHK(hipSetDevice(src.device));
        }
    }
    if (seconds) *seconds = s;
    return 0;
}

int table_subtract(Table &dst, Table &src, Table &minus, uint64_t out5[5], double *seconds, std::string &err) {
    if (!out5) { err = "subtract: null output"; return -1; }
    if (check_subtract(dst, src, minus, err)) return -1;
    uint64_t piece = 0;
    if (piece_slots("subtract", "JASPER_SUBTRACT_PIECE", piece, err)) return -1;
    HIPCHK(hipSetDevice(src.device));
    if (dst.materialize(err) || dst.read_stats(err)) return -1;
    if (dst.h_stats[ST_DISTINCT] != 0) { err = "subtract: the destination table must be empty (it holds " + std::to_string(dst.h_stats[ST_DISTINCT]) + " keys)"; return -1; }
    Table *others[2] = {&minus, &dst};
    Events order;
    if (settle(src, others, 2, order, err)) return -1;
    hipStream_t st = src.stream;
    const uint64_t cap = std::min<uint64_t>(piece, src.nslots);
    unsigned long long *d_ent = (unsigned long long *)src.workspace(Table::WS_SELECT, (size_t)cap * 3 * sizeof(unsigned long long), err);
    if (!d_ent) return -1;
    unsigned long long *d_ctl = (unsigned long long *)src.workspace(Table::WS_SELECT + 1, SUB_CTL * sizeof(unsigned long long), err);
    if (!d_ctl) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    double s = 0;
    unsigned long long occurrences = 0;
    for (int i = 0; i < SUB_NCOUNT; ++i) out5[i] = 0;
    for (uint64_t first = 0; first < src.nslots; first += piece) {
        const uint64_t end = std::min<uint64_t>(first + piece, src.nslots);
        HIPCHK(hipMemsetAsync(d_ctl, 0, SUB_CTL * sizeof(unsigned long long), st));
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(table_subtract_kernel, dim3(select_grid(end - first)), dim3(SP_THREADS), 0, st, src.d, minus.d, first, end, d_ent, (unsigned long long)cap, d_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        unsigned long long res[SUB_CTL];
        HIPCHK(hipMemcpyAsync(res, d_ctl, sizeof res, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        if (ev.add_seconds(s, err)) return -1;
        if (res[0] != res[1 + SUB_KEPT] || res[0] > end - first || res[1 + SUB_SWEPT] != res[1 + SUB_DROPPED] + res[1 + SUB_UNDERFLOW] + res[1 + SUB_KEPT]) {
            err = "subtract: a piece's entry count does not match its counters";
            return -1;
        }
        for (int i = 0; i < SUB_NCOUNT; ++i) out5[i] += res[1 + i];
        occurrences += res[1 + SUB_SUM];
        // (the kernel has finished: the destination's stream may read the entries, and has read them when import_entries returns)
        if (res[0]) {
            const int rc = dst.import_entries(d_ent, res[0], err);
            if (rc) return rc;
            HIPCHK(hipSetDevice(src.device));
        }
    }
    // an import adds no occurrences; a difference stands for the sequences src counts and minus does not, whose k-mer occurrences are its sum
    HIPCHK(hipMemcpyAsync(dst.d.stats + ST_OCCURRENCES, &occurrences, sizeof occurrences, hipMemcpyHostToDevice, dst.stream));
    if (dst.read_stats(err)) return -1;
    if (seconds) *seconds = s;
    return 0;
}

}  // namespace jk
