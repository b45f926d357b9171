// scan_tile.hip -- the parts of the dense scans' shared stage that are no templates (scan_tile.hpp): the heads kernel and the host side's
// text packing, the ordering of a scan's tables before its stream, and the tile list.
#include "scan_tile.hpp"

namespace jk {

constexpr int SH_THREADS = 1024;
__global__ __launch_bounds__(SH_THREADS) void scan_heads_kernel(const ScanTile *__restrict__ tiles, const TileRuns *__restrict__ tout, uint64_t ntiles,
                                                                unsigned long long *__restrict__ head_base, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long s_w[SH_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t per = (ntiles + SH_THREADS - 1) / SH_THREADS;
    const uint64_t lo = (uint64_t)t * per < ntiles ? (uint64_t)t * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    unsigned long long sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += tout[i].nruns - tile_continues(tiles, tout, i);
    const unsigned long long incl = wave_incl_scan(sum);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long at = incl - sum;
    for (int w = 0; w < wave; ++w) at += s_w[w];
    for (uint64_t i = lo; i < hi; ++i) {
        head_base[i] = at;
        at += tout[i].nruns - tile_continues(tiles, tout, i);
    }
    if (t == SH_THREADS - 1) ctl[SC_HEADS] = at;
}

int launch_heads(hipStream_t st, const ScanTile *d_tiles, const TileRuns *d_tout, uint64_t ntiles, unsigned long long *d_head, unsigned long long *d_ctl, std::string &err) {
    hipLaunchKernelGGL(scan_heads_kernel, dim3(1), dim3(SH_THREADS), 0, st, d_tiles, d_tout, ntiles, d_head, d_ctl);
    HIPCHK(hipGetLastError());
    return 0;
}

int pack_host_text(Table &T, int slot, int n_seqs, const char *const *seqs, const int64_t *lens, const char *what, HostText &H, std::string &err) {
    HIPCHK(hipSetDevice(T.device));
    H.offs.assign((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        if (lens[i] < 0 || (lens[i] && !seqs[i])) { err = std::string(what) + ": bad sequence"; return -1; }
        H.offs[i + 1] = H.offs[i] + lens[i];
    }
    const size_t total = (size_t)H.offs[n_seqs];
    H.d_text = (uint8_t *)T.workspace(slot, total + 16, err);
    if (!H.d_text) return -1;
    const char *src = n_seqs == 1 ? seqs[0] : nullptr;
    if (n_seqs > 1) {                       // one copy for many short sequences
        H.all.resize(total);
        for (int i = 0; i < n_seqs; ++i)
            if (lens[i]) memcpy(H.all.data() + H.offs[i], seqs[i], (size_t)lens[i]);
        src = H.all.data();
    }
    if (total) HIPCHK(hipMemcpyAsync(H.d_text, src, total, hipMemcpyHostToDevice, T.stream));
    return 0;
}

int settle(Table &T, Table *const *others, int n, Events &order, std::string &err) {
    if (T.materialize(err)) return -1;
    for (int i = 0; i < n; ++i)
        if (others[i] && others[i]->materialize(err)) return -1;
    HIPCHK(hipEventCreate(&order.e[0]));
    for (int i = 0; i < n; ++i) {
        if (!others[i] || others[i] == &T) continue;
        HIPCHK(hipEventRecord(order.e[0], others[i]->stream));
        HIPCHK(hipStreamWaitEvent(T.stream, order.e[0], 0));
    }
    return 0;
}

int build_tiles(int k, int n_seqs, const uint8_t *d_text, const int64_t *offsets, const char *what, uint64_t *per_seq, size_t stride, TileList &L, std::string &err) {
    const std::string w(what);
    for (int i = 0; i < n_seqs; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0) { err = w + ": offsets must not decrease"; return -1; }
        const int64_t n = offsets[i + 1] - offsets[i];
        const uint64_t nw = n >= k ? (uint64_t)(n - k + 1) : 0;
        if (per_seq) per_seq[stride * (size_t)i] = nw;
        L.windows += nw;
        const uint64_t nt = (nw + RP_TILE - 1) / RP_TILE;
        if (nt > 0xFFFFFFFFull) { err = w + ": sequence too long"; return -1; }
        for (uint64_t q = 0; q < nt; ++q) L.tiles.push_back(ScanTile{(uint32_t)i, (uint32_t)q});
    }
    if (!L.tiles.empty() && !d_text) { err = w + ": null text"; return -1; }
    return 0;
}

int upload_tiles(Table &T, int W, int n_seqs, const int64_t *offsets, TileList &L, std::string &err) {
    const size_t ntiles = L.tiles.size();
    L.d_offs = (int64_t *)T.workspace(W + 1, ((size_t)n_seqs + 1) * sizeof(int64_t), err);
    L.d_tiles = (ScanTile *)T.workspace(W + 2, ntiles * sizeof(ScanTile), err);
    if (!L.d_offs || !L.d_tiles) return -1;
    HIPCHK(hipMemcpyAsync(L.d_offs, offsets, ((size_t)n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, T.stream));
    HIPCHK(hipMemcpyAsync(L.d_tiles, L.tiles.data(), ntiles * sizeof(ScanTile), hipMemcpyHostToDevice, T.stream));
    return 0;
}

}  // namespace jk
