// variants.hip -- variant scan: the positions of every sequence where the reads hold a solid single-base alternative to the base the
// sequence has, as per-sequence counters and one record per (position, alternative) (semantics: include/jasper_hip.h,
// jasper_variant_scan).
//
// An extension.  The reference meets the situation inside its walk (src/jasper.py: fixdiploid, fix_k_case_sub) and reports nothing;
// this is the dense scan of report.hip asking another question of the same table: not "is this window's k-mer there" but "would it
// be there with another last base".
//
//   variants_scan_kernel     the dense scans' tile (scan_tile.hpp: staging, the rolling state before a thread's first window).  The halo
//                            is 128 bases, not 64: a position p is `evaluated` when the 2k - 1 bytes around it are bases, which the
//                            thread that owns byte p + k - 1 sees as a run of at least 2k - 1 bases ending there (up to 127 back).
//                            For a valid window that ends at p the three alternatives of its last base come from the rolling state
//                            (fwd ^ d in the low bit pair, rc ^ (d << 2(k-1)), d = 1, 2, 3: (3-a) ^ (3-b) = a ^ b); each is
//                            canonicalised, mixed and probed.  The base the sequence has is NOT probed here.  An alternative with
//                            count >= thre makes (seq, p, alt) a CANDIDATE: that is the j = 0 term of the minimum over the k windows
//                            that cover p, hence necessary.  VS_BATCH windows' home-slot loads (3 each) are in flight before any is
//                            resolved (DESIGN 4.6 has the register figures of 4, 2 and 1).  A thread's candidates are a 48-bit mask;
//                            places in the list are reserved as every dense scan reserves them (scan_tile.hpp: a block-wide scan, one
//                            cursor add per tile).  One more add per tile counts the evaluated positions of the sequence.
//   variants_check_kernel    one wave per candidate, lane j < k owns the window that starts at p - k + 1 + j.  The wave loads the
//                            2k - 1 context bytes once (lane l: bytes l and l + 64); the candidate is dropped unless p <= n - k and
//                            all of them are bases.  Each lane gathers its k-mer from the wave's registers, forms it with the
//                            alternative (fwd ^ (d << 2j), rc ^ (d << 2(k-1-j))), looks both up through table_get; two wave-wide
//                            minima; lane 0 writes the record, or kind 0, into the candidate's own slot.
//   variants_compact_kernel  the accepted records to the front of a second list, one cursor add per wave.  Their order there is that of
//                            arrival; the host sorts the (small) accepted list by (seq, pos, alt), a unique key.
//
// The candidate list starts at windows / 64 + 64K entries; a scan that found more has counted them and is repeated once with exactly
// that room (run_counted in scan_tile.hpp, where the text packing and the tile list are too).  The host side is two stages --
// variant_scan_stage (tiles, scan, retry) and variant_check_stage (check, compact, sort) -- because the indel scan (indels.hip) runs the
// first, its own check over the raw candidates, and then the second.
#include "variants.hpp"
#include "scan_tile.hpp"

#ifndef VS_BATCH
#define VS_BATCH 2             // windows whose three home-slot loads are in flight together: 4, 2 or 1
#endif
#ifndef VS_BATCH_UNROLL
#define VS_BATCH_UNROLL 1      // 1: a thread's batches as a loop
#endif
#define VS_STR_(x) #x
#define VS_PRAGMA_UNROLL(n) _Pragma(VS_STR_(unroll n))

namespace jk {

static_assert(VS_BATCH == 1 || VS_BATCH == 2 || VS_BATCH == 4, "VS_BATCH divides a thread's 16 windows");
constexpr int VS_HALO = 8;                                               // groups of 16 bases staged before a tile: 128 >= 2k - 1
enum { VC_ACCEPTED = 1 };                                                // control word 1: records accepted

__global__ __launch_bounds__(RP_THREADS) void variants_scan_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, const ScanTile *__restrict__ tiles,
                                                                   uint64_t ntiles, TableDev R, uint32_t thre, unsigned long long *__restrict__ counts,
                                                                   Variant *__restrict__ cand, unsigned long long cap, unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t s_code[RP_THREADS + VS_HALO];
    __shared__ uint32_t s_inv[RP_THREADS + VS_HALO];
    __shared__ uint32_t s_wsum[RP_THREADS / 64];
    __shared__ uint32_t s_eval;                         // evaluated positions of the tile
    __shared__ unsigned long long s_base;
    const int t = threadIdx.x, lane = t & 63;
    const int k = R.k;
    const u128 kmask = maskbits(2 * k);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const ScanTile D = tiles[tile];
        if (t == 0) s_eval = 0;
        int64_t n, w0, e0;
        uint32_t c, iv;
        u128 fwd, rc;
        int run;                                        // bases in a row that end right before my first one, up to 128
        tile_prologue<VS_HALO>(text, offs, D, k, kmask, s_code, s_inv, n, w0, e0, c, iv, fwd, rc, run);
        unsigned long long cm = 0;                      // bit 3j + d - 1: the window that ends at e0 + j with its last base ^ d is solid
        uint32_t evm = 0;                               // bit j: the position k - 1 before e0 + j is evaluated
        VS_PRAGMA_UNROLL(VS_BATCH_UNROLL)
        for (int j0 = 0; j0 < RP_GROUP; j0 += VS_BATCH) {
            u128 hs[VS_BATCH * 3];
            ulonglong2 er[VS_BATCH * 3];
            bool ok[VS_BATCH];
#pragma unroll
            for (int u = 0; u < VS_BATCH; ++u) {
                const int j = j0 + u;
                const uint32_t cj = (c >> (30 - 2 * j)) & 3u;
                const bool bad = (iv >> (15 - j)) & 1u;
                fwd = band(bor(shl(fwd, 2), mk(0, cj)), kmask);
                rc = bor(shr(rc, 2), shl(mk(0, 3u - cj), 2 * (k - 1)));
                run = bad ? 0 : run + 1;
                ok[u] = run >= k && e0 + j < n;
                evm |= (run >= 2 * k - 1 && e0 + j < n ? 1u : 0u) << j;
#pragma unroll
                for (int d = 1; d < 4; ++d) {
                    const u128 fa = bxor(fwd, mk(0, (uint64_t)d));
                    const u128 ra = bxor(rc, shl(mk(0, (uint64_t)d), 2 * (k - 1)));
                    const u128 h = mix(lt(ra, fa) ? ra : fa, R.B);
                    hs[3 * u + d - 1] = h;
                    er[3 * u + d - 1] = make_ulonglong2(0ull, 0ull);
                    if (ok[u]) er[3 * u + d - 1] = *reinterpret_cast<const ulonglong2 *>(read_slots(R, h) + 2 * home_of(h, R.B, R.s));
                }
            }
#pragma unroll
            for (int u = 0; u < VS_BATCH; ++u) {
#pragma unroll
                for (int d = 1; d < 4; ++d) {
                    const uint32_t cnt = ok[u] ? clamp32(table_get_prefetched(R, hs[3 * u + d - 1], er[3 * u + d - 1])) : 0u;
                    cm |= (unsigned long long)(cnt >= thre ? 1u : 0u) << (3 * (j0 + u) + d - 1);      // (thre >= 1: never where there is no window)
                }
            }
        }
        {
            const uint32_t ce = wave_sum(__popc(evm));
            if (lane == 0 && ce) atomicAdd(&s_eval, ce);
        }
        const uint32_t ns = __popcll(cm);
        const TileSlots S = tile_reserve(ns, s_wsum, &s_base, &ctl[SC_CURSOR]);
        if (t == 0 && s_eval) atomicAdd(&counts[D.seq], (unsigned long long)s_eval);
        unsigned long long at;
        if (tile_granted(S, &s_base, cap, at)) {
            while (cm) {
                const int b = __builtin_ctzll(cm);
                cm &= cm - 1;
                const int j = b / 3, d = b - 3 * j + 1;
                Variant v;
                v.pos = e0 + j;
                v.seq = D.seq;
                v.ref_min = 0;
                v.alt_min = 0;
                v.ref = 0;
                v.alt = (uint8_t)(((c >> (30 - 2 * j)) & 3u) ^ (uint32_t)d);      // the alternative's code; the check turns it into a letter
                v.kind = VK_REJECTED;
                v.pad = 0;
                cand[at++] = v;
            }
        }
        __syncthreads();      // (the next tile reuses the LDS arrays)
    }
}

__global__ __launch_bounds__(256) void variants_check_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, TableDev R, uint32_t thre, Variant *cand,
                                                             uint64_t ncand) {
    const int lane = threadIdx.x & 63;
    const int k = R.k;
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ncand; i += nwv) {
        const int64_t p = cand[i].pos;
        const uint32_t seq = cand[i].seq;
        const uint32_t alt = cand[i].alt & 3u;
        const int64_t o0 = offs[seq];
        const int64_t n = offs[seq + 1] - o0;
        const uint8_t *__restrict__ txt = text + o0;
        bool keep = p >= k - 1 && p <= n - k;           // (wave-uniform) all k windows that cover p exist: bytes p - k + 1 .. p + k - 1 are inside
        int c0 = -1, c1 = -1;                           // codes of context bytes lane and lane + 64
        if (keep) {
            const int64_t b0 = p - k + 1;
            const bool in0 = lane < 2 * k - 1, in1 = lane + 64 < 2 * k - 1;
            if (in0) c0 = code(txt[b0 + lane]);
            if (in1) c1 = code(txt[b0 + lane + 64]);
            keep = __ballot((in0 && c0 < 0) || (in1 && c1 < 0)) == 0ull;
        }
        uint32_t rmin = 0xFFFFFFFFu, amin = 0xFFFFFFFFu;
        uint32_t refc = 0;
        if (keep) {
            refc = (uint32_t)__shfl(c0, k - 1) & 3u;
            u128 fwd = mk(0, 0);
            for (int q = 0; q < k; ++q) {               // my window's base q is context byte lane + q (lanes >= k gather bytes nobody uses)
                const int idx = lane + q;
                const int v0 = __shfl(c0, idx & 63), v1 = __shfl(c1, idx & 63);
                fwd = bor(shl(fwd, 2), mk(0, (uint64_t)((idx < 64 ? v0 : v1) & 3)));
            }
            if (lane < k) {
                const u128 rc = revcomp(fwd, k);
                const uint64_t d = refc ^ alt;          // p is my window's base k - 1 - lane: bit pair `lane` of fwd, k - 1 - lane of rc
                const u128 fa = bxor(fwd, shl(mk(0, d), 2 * lane));
                const u128 ra = bxor(rc, shl(mk(0, d), 2 * (k - 1 - lane)));
                rmin = clamp32(table_get(R, mix(lt(rc, fwd) ? rc : fwd, R.B)));
                amin = clamp32(table_get(R, mix(lt(ra, fa) ? ra : fa, R.B)));
            }
            rmin = wave_min32(rmin);
            amin = wave_min32(amin);
        }
        if (lane == 0) {
            const bool solid = keep && amin >= thre;
            Variant v;
            v.pos = p;
            v.seq = seq;
            v.ref_min = solid ? rmin : 0u;
            v.alt_min = solid ? amin : 0u;
            v.ref = (uint8_t)((0x54474341u >> (8 * refc)) & 0xFFu);       // "ACGT"
            v.alt = (uint8_t)((0x54474341u >> (8 * alt)) & 0xFFu);
            v.kind = !solid ? VK_REJECTED : rmin >= thre ? VK_HET : VK_ERROR;
            v.pad = 0;
            cand[i] = v;
        }
    }
}

__global__ __launch_bounds__(256) void variants_compact_kernel(const Variant *__restrict__ cand, uint64_t ncand, Variant *__restrict__ out,
                                                               unsigned long long *__restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < ncand; i0 += stride) {      // (i0: the wave's first, so a wave stays together)
        const uint64_t i = i0 + lane;
        const bool acc = i < ncand && cand[i].kind != VK_REJECTED;
        const unsigned long long m = __ballot(acc);
        if (m == 0ull) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&ctl[VC_ACCEPTED], (unsigned long long)__popcll(m));
        base = __shfl(base, 0);
        if (acc) out[base + __popcll(m & ((1ull << lane) - 1ull))] = cand[i];
    }
}

// The scan stage that the variant scan and the indel scan (indels.hip) share: the tile list, the launch of variants_scan_kernel, and the
// retry with exactly the counted room.  On return S names the candidate list and the per-sequence counters in the workspace; ntiles == 0
// (nothing to scan) leaves the rest of S unset.  `what` starts the error messages.
int variant_scan_stage(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, const char *what, VariantOut &out, VariantStage &S,
                       std::string &err) {
    S = VariantStage();
    TileList L;
    if (build_tiles(T.k, n_seqs, d_text, offsets, what, nullptr, 0, L, err)) return -1;
    const uint64_t ntiles = L.tiles.size();
    if (ntiles == 0) return 0;
    hipStream_t st = T.stream;
    const int W = Table::WS_VARIANTS;
    const size_t cnt_words = (size_t)n_seqs + SC_WORDS;
    unsigned long long *d_cnt = (unsigned long long *)T.workspace(W + 3, cnt_words * sizeof(unsigned long long), err);
    if (!d_cnt || upload_tiles(T, W, n_seqs, offsets, L, err)) return -1;
    unsigned long long *d_ctl = d_cnt + (size_t)n_seqs, ctl[SC_WORDS] = {0, 0, 0, 0};
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 256 * 8);
    Variant *d_cand = nullptr;
    auto scan = [&](unsigned long long cap) {
        d_cand = (Variant *)T.workspace(W + 4, cap * sizeof(Variant), err);
        if (!d_cand) return -1;
        hipLaunchKernelGGL(variants_scan_kernel, dim3(grid), dim3(RP_THREADS), 0, st, d_text, L.d_offs, L.d_tiles, ntiles, T.d, thre, d_cnt, d_cand, cap, d_ctl);
        return 0;
    };
    if (run_counted(st, d_cnt, cnt_words, d_ctl, L.windows / 64 + 65536, std::string(what) + ": the number of candidates changed between two scans", ctl, out.seconds,
                    out.retried, err, scan))
        return -1;
    S.ntiles = ntiles;
    S.ncand = ctl[SC_CURSOR];
    S.d_offs = L.d_offs;
    S.d_cnt = d_cnt;
    S.d_ctl = d_ctl;
    S.d_cand = d_cand;
    out.candidates = S.ncand;
    return 0;
}

// The check stage: variants_check_kernel over the candidates of S (it rewrites them in place), variants_compact_kernel, the sort and the
// counters.
int variant_check_stage(Table &T, int n_seqs, const uint8_t *d_text, uint32_t thre, const char *what, const VariantStage &S, VariantOut &out, std::string &err) {
    const std::string w(what);
    hipStream_t st = T.stream;
    const uint64_t ncand = S.ncand;
    unsigned long long ctl[SC_WORDS] = {0, 0, 0, 0};
    std::vector<unsigned long long> cnt((size_t)n_seqs);
    HIPCHK(hipMemcpyAsync(cnt.data(), S.d_cnt, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (ncand) {
        Events ev;
        if (ev.create(err)) return -1;
        Variant *d_out = (Variant *)T.workspace(Table::WS_VARIANTS + 5, ncand * sizeof(Variant), err);
        if (!d_out) return -1;
        HIPCHK(hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(variants_check_kernel, dim3((unsigned)std::min<uint64_t>((ncand + 3) / 4, 256 * 16)), dim3(256), 0, st, d_text, S.d_offs, T.d, thre, S.d_cand, ncand);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(variants_compact_kernel, dim3((unsigned)std::min<uint64_t>((ncand + 255) / 256, 256 * 8)), dim3(256), 0, st, S.d_cand, ncand, d_out, S.d_ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.e[1], st));
        HIPCHK(hipMemcpyAsync(ctl, S.d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        if (ev.add_seconds(out.seconds, err)) return -1;
        const uint64_t nrec = ctl[VC_ACCEPTED];
        if (nrec > ncand) { err = w + ": more records than candidates"; return -1; }
        out.recs.resize(nrec);
        if (nrec) HIPCHK(hipMemcpyAsync(out.recs.data(), d_out, nrec * sizeof(Variant), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(jk_stream_wait(st));
    std::sort(out.recs.begin(), out.recs.end(), [](const Variant &a, const Variant &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.pos != b.pos ? a.pos < b.pos : a.alt < b.alt;      // ('A' < 'C' < 'G' < 'T')
    });
    for (int i = 0; i < n_seqs; ++i) out.counts[3 * (size_t)i] = cnt[(size_t)i];
    for (const Variant &v : out.recs) {
        if (v.seq >= (uint32_t)n_seqs || (v.kind != VK_HET && v.kind != VK_ERROR)) { err = w + ": a record the check cannot have written"; return -1; }
        ++out.counts[3 * (size_t)v.seq + v.kind];
    }
    return 0;
}

int variant_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, VariantOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "variant scan: bad arguments"; return -1; }
    if (thre < 1) { err = "variant scan: the threshold must be at least 1"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    if (T.materialize(err)) return -1;       // a logically empty table holds garbage until it is zeroed
    out.counts.assign((size_t)n_seqs * 3, 0);
    out.recs.clear();
    out.candidates = 0;
    out.seconds = 0;
    out.retried = 0;
    VariantStage S;
    if (variant_scan_stage(T, n_seqs, d_text, offsets, thre, "variant scan", out, S, err)) return -1;
    if (S.ntiles == 0) return 0;
    return variant_check_stage(T, n_seqs, d_text, thre, "variant scan", S, out, err);
}

int variant_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, VariantOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "variant scan: bad arguments"; return -1; }
    if (thre < 1) { err = "variant scan: the threshold must be at least 1"; return -1; }
    HostText H;
    if (pack_host_text(T, Table::WS_VARIANTS, n_seqs, seqs, lens, "variant scan", H, err)) return -1;
    return variant_scan_device(T, n_seqs, H.d_text, H.offs.data(), thre, out, err);
}

}  // namespace jk
