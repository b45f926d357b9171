// compound.hip -- compound scan: what the reads hold in place of a cluster of differences that hide each other from the variant and the
// indel scan (semantics: include/jasper_hip.h, jasper_compound_scan).
//
// An extension.  The reference repairs such clusters inside its walk, one difference at a time where it can, and reports nothing.  The
// dense scan is the report's (report.hip), unchanged: a maximal run of n_kmers >= k unreliable windows is what R = n_kmers - k + 1 bytes
// of the sequence leave when no window that holds one of them is solid.  The host picks those runs (R <= max_len: a site; longer ones are
// counted), uploads them as plain (seq, a, q, ref_min) tuples and launches
//
//   compound_search_kernel   one wave per site, four per block, grid-stride: a front search on the shared pieces of front_search.hpp
//                            (DESIGN 4.8.1).  F = the k - 1 bases before a and G = the k - 1 bases from q on are two wave-uniform
//                            128-bit words (front_flanks; a flank out of bounds or with a non-base: no search).  The frontier S_t is
//                            at most COMPOUND_FRONT = 64 prefixes of the replacement y, one per lane -- y of up to 64 bases as 2-bit
//                            codes in 128 bits, first base in the highest pair, so that lane order is lexicographic order -- with
//                            the minimum over its t windows.  The kernel's own part of each shared step:
//                              extend   (front_extend, front_handover) the child's newest window is the last k bases of F + y + z:
//                                       ((F << 2t) | yz) & mask(2k) while t < k and yz & mask(2k) from t >= k on (F << 2t is formed
//                                       only for t < k <= 64, so no shift reaches 128 bits).  The strip is 64 x (16 + 4) bytes per
//                                       wave.  More than 64 children: the site is complex, counted once, and the wave stops there.
//                              rejoin   (front_window0, front_rejoin with front_window) from W = the last k - 1 bases of F + y (y
//                                       alone from t >= k - 1 on)
//                              records  (front_reserve) lane i its own.  Level 1 of a site with R = 1 is searched but not listed: it
//                                       is the variant scan's.
//
// The record list starts at sites + 4096 entries; a search that found more has counted them and is repeated once with exactly that room
// (search_stage and run_counted, scan_tile.hpp).  The dense scan is not repeated.
#include "compound.hpp"
#include "front_search.hpp"

namespace jk {

enum { CC_LOOKUPS = 1, CC_COMPLEX = 2 };                                 // control words 1 and 2: table lookups made; complex sites

__global__ __launch_bounds__(256) void compound_search_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ offs, uint32_t n_seqs, TableDev R, uint32_t thre,
                                                              int max_len, const CompoundSite *__restrict__ sites, uint64_t nsites, Compound *__restrict__ out,
                                                              unsigned long long cap, unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ cplx) {
    __shared__ ulonglong2 s_y[4][COMPOUND_FRONT];       // a wave's next frontier: y (.x low, .y high) ...
    __shared__ uint32_t s_mn[4][COMPOUND_FRONT];        // ... and its running minimum
    const int lane = threadIdx.x & 63;
    ulonglong2 *strip_y = s_y[threadIdx.x >> 6];
    uint32_t *strip_mn = s_mn[threadIdx.x >> 6];
    const int k = R.k;
    const u128 kmask = maskbits(2 * k), fmask = maskbits(2 * (k - 1));
    const uint64_t nwv = (uint64_t)gridDim.x * 4;
    unsigned long long nlook = 0, ncomplex = 0;         // (wave-uniform)
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nsites; i += nwv) {
        const CompoundSite S = sites[i];
        if (S.seq >= n_seqs) continue;                  // (wave-uniform, like every check here; the host writes no such site)
        const int64_t o0 = offs[S.seq];
        const int64_t n = offs[S.seq + 1] - o0;
        const int64_t RL = S.q - S.a;
        if (S.a < k - 1 || RL < 1 || RL > max_len || S.q > n - (k - 1)) continue;      // F and G lie inside the sequence
        const Flanks FG = front_flanks(text + o0, S.a, S.q, k);
        if (!FG.bases) continue;                        // ... and are bases
        const u128 F = FG.F, G = FG.G;
        // level 0: S_0 = {empty}
        u128 y = mk(0, 0);                              // lane i < nf: prefix i, first base in the highest pair ...
        uint32_t mn = 0xFFFFFFFFu;                      // ... and the minimum over its windows
        int nf = 1;
        for (int t = 1; t <= max_len; ++t) {
            // extend S_(t-1) to S_t: the last k bases of F + y + z
            const u128 Fs = t < k ? shl(F, 2 * t) : mk(0, 0);      // from t >= k on the newest window is y's alone (and 2t may be 128)
            const int tot = front_extend(
                R, thre, y, mn, nf, COMPOUND_FRONT,
                [=](int, u128 parent) {
                    const u128 ny = bor(shl(parent, 2), mk(0, (uint64_t)(lane & 3)));      // (t - 1 <= 63 bases: nothing is lost)
                    return FrontChild<u128>{ny, band(bor(Fs, ny), kmask), true, true};
                },
                [&](int at, int, u128 ny, uint32_t m) {
                    strip_y[at] = make_ulonglong2(ny.lo, ny.hi);
                    strip_mn[at] = m;
                });
            nlook += 4u * (unsigned)nf;
            if (tot > COMPOUND_FRONT) {                 // complex: nothing of length >= t is listed here
                ++ncomplex;
                if (lane == 0) atomicAdd(&cplx[S.seq], 1ull);
                break;
            }
            if (tot == 0) break;
            front_handover(tot, [&](int l) {
                const ulonglong2 v = strip_y[l];
                y = mk(v.y, v.x);
                mn = strip_mn[l];
            });
            nf = tot;
            if (RL == 1 && t == 1) continue;            // a single substitution: the variant scan's
            // rejoin: window t, lane i for prefix i
            const bool act = lane < nf;
            const u128 W = t >= k - 1 ? band(y, fmask) : band(bor(Fs, y), fmask);      // the last k - 1 bases of F + y  (t < k - 1: Fs = F << 2t)
            uint32_t a = 0xFFFFFFFFu;
            if (act) a = canon_count(R, front_window0(W, G, k, kmask), k);
            nlook += (unsigned)nf;
            a = min32(a, mn);
            uint32_t my_amin;
            const unsigned long long recm = front_rejoin(R, thre, __ballot(act && a >= thre), a, nlook, my_amin, [&](int j) { return front_window(readlane128(W, j), G, k, kmask); });
            if (recm) {
                const unsigned long long at = front_reserve(recm, &ctl[SC_CURSOR], cap);
                if (at != FRONT_NONE) {
                    const u128 rv = shr(mk(revpairs64(y.lo), revpairs64(y.hi)), 128 - 2 * t);      // base i in bits 2i, 2i + 1
                    Compound v;
                    v.pos = S.a;
                    v.seq = S.seq;
                    v.ref_min = S.ref_min;
                    v.alt_min = my_amin;
                    v.ref_len = (uint32_t)RL;
                    v.bases[0] = rv.lo;
                    v.bases[1] = rv.hi;
                    v.len = (uint16_t)t;
                    for (int z = 0; z < 6; ++z) v.pad[z] = 0;
                    out[at] = v;
                }
            }
        }
    }
    if (lane == 0 && nlook) atomicAdd(&ctl[CC_LOOKUPS], nlook);
    if (lane == 0 && ncomplex) atomicAdd(&ctl[CC_COMPLEX], ncomplex);
}

static int compound_check_args(const Table &T, uint32_t thre, int max_len, std::string &err) {
    if (thre < 1) { err = "compound scan: the threshold (thre) must be at least 1"; return -1; }
    if (T.k < 2) { err = "compound scan: k must be at least 2"; return -1; }
    if (max_len < 1 || max_len > COMPOUND_MAX_LEN) { err = "compound scan: max_len must be in 1..64"; return -1; }
    return 0;
}

// base i of a record's y
static inline unsigned compound_base(const Compound &v, int i) { return (unsigned)(v.bases[i >> 5] >> (2 * (i & 31))) & 3u; }

int compound_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, ReportOut &report, CompoundOut &out,
                         std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "compound scan: bad arguments"; return -1; }
    if (compound_check_args(T, thre, max_len, err)) return -1;
    out = CompoundOut();
    if (kmer_report_device(T, n_seqs, d_text, offsets, thre, report, err)) return -1;
    out.counts.assign((size_t)n_seqs * 5, 0);
    out.seconds = report.seconds;
    const uint64_t k = (uint64_t)T.k;
    std::vector<CompoundSite> sites;                    // in (seq, a) order, as the runs are
    for (const KmerRun &r : report.runs) {
        if (r.n_kmers < k) continue;                    // a pure insertion, an edge or a non-base byte: the other scans'
        if (r.seq >= (uint32_t)n_seqs) { err = "compound scan: a run of no sequence"; return -1; }
        if (r.n_kmers - k + 1 > (uint64_t)max_len) {
            ++out.counts[5 * (size_t)r.seq + 3];
            continue;
        }
        ++out.counts[5 * (size_t)r.seq + 0];
        sites.push_back(CompoundSite{r.start + (int64_t)k - 1, r.start + (int64_t)r.n_kmers, r.seq, r.min_count});
    }
    const uint64_t nsites = sites.size();
    if (nsites == 0) return 0;                          // nothing of the search is allocated or launched
    hipStream_t st = T.stream;
    const int W = Table::WS_COMPOUND;
    CompoundSite *d_sites = (CompoundSite *)T.workspace(W, nsites * sizeof(CompoundSite), err);
    int64_t *d_offs = (int64_t *)T.workspace(W + 1, ((size_t)n_seqs + 1) * sizeof(int64_t), err);
    if (!d_sites || !d_offs) return -1;
    HIPCHK(hipMemcpyAsync(d_sites, sites.data(), nsites * sizeof(CompoundSite), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_offs, offsets, ((size_t)n_seqs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    unsigned long long ctl[SC_WORDS] = {0, 0, 0, 0};
    std::vector<unsigned long long> cplx;               // after the control words: the complex sites per sequence
    const int sums[1] = {CC_COMPLEX};
    if (search_stage(T, W + 3, n_seqs, 1, sums, nsites + 4096, "compound scan: the number of records changed between two searches",
                     "compound scan: the complex sites per sequence do not add up", ctl, out.recs, cplx, out.search_seconds, out.retried, err,
                     [&](unsigned long long cap, unsigned long long *d_ctl, unsigned long long *d_per) {
                         Compound *d_rec = (Compound *)T.workspace(W + 2, cap * sizeof(Compound), err);
                         if (d_rec)
                             hipLaunchKernelGGL(compound_search_kernel, dim3((unsigned)std::min<uint64_t>((nsites + 3) / 4, 256 * 16)), dim3(256), 0, st, d_text, d_offs,
                                                (uint32_t)n_seqs, T.d, thre, max_len, d_sites, nsites, d_rec, cap, d_ctl, d_per);
                         return d_rec;
                     }))
        return -1;
    out.seconds += out.search_seconds;
    out.lookups = ctl[CC_LOOKUPS];
    for (size_t i = 0; i < cplx.size(); ++i) out.counts[5 * i + 4] = cplx[i];
    for (const Compound &v : out.recs) {                // a record the kernel cannot have written is refused
        const auto s = std::lower_bound(sites.begin(), sites.end(), v, [](const CompoundSite &a, const Compound &b) { return a.seq != b.seq ? a.seq < b.seq : a.a < b.pos; });
        bool ok = s != sites.end() && s->seq == v.seq && s->a == v.pos && (int64_t)v.ref_len == s->q - s->a && v.len >= 1 && (int)v.len <= max_len;
        if (ok && v.len < 32) ok = (v.bases[0] >> (2 * v.len)) == 0 && v.bases[1] == 0;
        if (ok && v.len >= 32 && v.len < 64) ok = (v.bases[1] >> (2 * (v.len - 32))) == 0;
        if (!ok) { err = "compound scan: a record the search cannot have written"; return -1; }
    }
    std::sort(out.recs.begin(), out.recs.end(), [](const Compound &a, const Compound &b) {
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.len != b.len) return a.len < b.len;
        for (int i = 0; i < (int)a.len; ++i)
            if (compound_base(a, i) != compound_base(b, i)) return compound_base(a, i) < compound_base(b, i);
        return false;
    });
    for (size_t i = 0; i < out.recs.size(); ++i) {
        const Compound &v = out.recs[i];
        ++out.counts[5 * (size_t)v.seq + 2];
        if (i == 0 || out.recs[i - 1].seq != v.seq || out.recs[i - 1].pos != v.pos) ++out.counts[5 * (size_t)v.seq + 1];
    }
    return 0;
}

int compound_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, ReportOut &report, CompoundOut &out,
                       std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "compound scan: bad arguments"; return -1; }
    if (compound_check_args(T, thre, max_len, err)) return -1;
    HostText H;
    if (pack_host_text(T, Table::WS_REPORT, n_seqs, seqs, lens, "compound scan", H, err)) return -1;
    return compound_scan_device(T, n_seqs, H.d_text, H.offs.data(), thre, max_len, report, out, err);
}

}  // namespace jk
