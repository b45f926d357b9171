// polish.hip -- the assembly scan / lookup / fix loop on the GPU.
//
// One 64-lane wavefront walks one SEGMENT of a chunk record (">name:offset", src/jasper.sh:155) through one pass
// of src/jasper.py:iteration.  The walk is sequential by definition (the next position depends on the last
// repair), so parallelism comes from these places:
//   * chunks are independent (the reference's own xargs -P parallelism, src/jasper.sh:212);
//   * a chunk is cut at sync points -- starts of runs of >= k-1 bad k-mers preceded by >= 4k clean positions, found
//     by a dense scan (scan_batch_kernel / classify_batch_kernel / find_sync_batch_kernel).  Any stride phase lands inside such a run
//     and handle_bad_kmers() then finds the same run bounds, so the walk right of a sync point is independent of
//     everything left of it except a coordinate shift: segments are walked concurrently and stitched afterwards.
//     A walk that touches text outside what its segment may assume raises spec_fail and the chunk is redone as one
//     segment (= the plain sequential walk);
//   * where sync points are scarce (later passes), a chunk is also cut inside long CLEAN stretches; the segment to the
//     right of such a cut takes its start position from the arrival position its left neighbour publishes (waves take
//     segments by ticket, so the neighbour is already running), and a segment whose range holds no event at all
//     computes its arrival instead of walking;
//   * the position classes are computed densely only in pass 0; afterwards the stitch carries the classes of
//     untouched windows over and rescan_batch_kernel recomputes the 64-window tiles next to edited text;
//   * inside a chunk the wave evaluates 64 stride positions i, i+(k-1), ... at once, ballots "needs
//     attention" and jumps to the first such position (positions that are plainly good only ever do
//     `i += k-1`, src/jasper.py:97,100);
//   * inside a repair the independent lookups (backward/forward run scans, check_sequence samples, dense
//     bad-k-mer counts, the four extensions of every live path) are spread over the lanes and reduced by
//     ballot / popcount.
// Everything else is executed uniformly by all 64 lanes (same values in every lane), i.e. as scalar code.
// The chunk text lives in a gap buffer in HBM so that `seq = seq[:a] + patch + seq[b:]` costs O(distance).
//
// Reference lines are cited as src/jasper.py:N.  Lookups go to the HBM table with the truncate-and-pad
// semantics of MerDNA(str) (Appendix A.3 of SURVEY.md; JF::include/jellyfish/mer_dna.hpp:525-542).
#include "polish.hpp"
#include <algorithm>

namespace jk {

constexpr int SMAX = 384;  // longest trial string kept in LDS (k <= 64: < 4k + 64)

__device__ __forceinline__ void pyslice(int64_t len, int64_t a, int64_t b, int64_t &lo, int64_t &hi) {
    if (a < 0) { a += len; if (a < 0) a = 0; } else if (a > len) a = len;
    if (b < 0) { b += len; if (b < 0) b = 0; } else if (b > len) b = len;
    if (b < a) b = a;
    lo = a; hi = b;
}

// Python round(): half-to-even on the double (device rint under the default rounding mode)
__device__ __forceinline__ int64_t pyround(double x) { return (int64_t)rint(x); }

struct FrontEntry {       // live path of the extension search
    uint32_t node;        // trie node of its last base
    uint16_t tlen;        // valid bytes in tail
    uint8_t alive;
    uint8_t pad;
    uint8_t tail[72];     // last min(len, k+3) bytes of start_km1 + path
};
static_assert(sizeof(FrontEntry) == 80, "FrontEntry layout");

// The walk's phase timers (SegDev::tk: how a segment's time splits into skipping good k-mers / finding the run / choosing a fix /
// splicing) read the clock around every step of the walk: a tuning aid that costs registers, scratch and an instruction stream
// the product does not need.  They are compiled in by `make EXTRA=-DJK_POLISH_TICKS=1` (JASPER_POLISH_DEBUG then prints the
// breakdown; without it the breakdown reads zero); a segment's total time (SegDev::ticks, two clock reads) is always there.
#ifndef JK_POLISH_TICKS
#define JK_POLISH_TICKS 0
#endif
__device__ __forceinline__ uint64_t phase_clock() { return JK_POLISH_TICKS ? wall_clock64() : 0ull; }

struct Walker {
    TableDev T;
    int k, step, lane;
    uint32_t solid;
    uint8_t *buf;
    int64_t len, gs, glen, cap;
    SegDev *C;
    uint32_t chunk_id;
    uint32_t nrec, naux, seqno, nedit;
    int pass;
    int status;
    uint64_t nlook;
    uint64_t tk[12];
    uint8_t *s_tbf, *s_t1, *s_t2, *s_gkb, *s_gka;
    // segment context
    int64_t delta;        // len - len0: how far text right of the last edit has shifted
    int64_t dirty_end;    // local positions >= dirty_end hold pass-start text (shifted by delta)
    int64_t glo;          // reads below this local position are outside what a non-first segment may assume
    bool is_first, is_last;
    int spec_fail;
    const uint8_t *cls;
    int64_t cls_n, seg_lo, stop_orig;
    ScratchPool pool;
    // path-search scratch (valid while a pool slot is held)
    uint32_t *bfs_nodes;
    uint8_t *bfs_front, *bfs_patch;
    int bfs_slot;

    // a read of local range [lo, hi) (pre-clamp bounds) must stay inside what this segment knows to be true text
    __device__ __forceinline__ void guard(int64_t lo, int64_t hi) {
        if ((!is_first && lo < glo) || (!is_last && hi > len)) spec_fail = 1;
    }

    // ---------------- text access ----------------
    __device__ __forceinline__ uint8_t at(int64_t p) const { return buf[p < gs ? p : p + glen]; }

    // 16 bytes at an arbitrary byte address (gfx950 runs with unaligned global access enabled)
    struct __attribute__((packed, aligned(1))) U16 { uint32_t w[4]; };

    // the (up to 64) text bytes [lo, lo+n) into registers with at most four 16-B loads that are all in flight together.
    // (Reading the window byte by byte in a loop that stops at the first non-ACGT base serialises k load latencies --
    // that was most of the time of every fix.)
    __device__ __forceinline__ void load_window(int64_t lo, int n, uint32_t w[16]) const {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t s = lo + 16 * c;
            U16 v;
            v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
            if (16 * c < n) {
                if (s + 16 <= gs) v = *reinterpret_cast<const U16 *>(buf + s);
                else if (s >= gs && s + glen + 16 <= cap) v = *reinterpret_cast<const U16 *>(buf + s + glen);
                else {                                   // straddles the gap or the end of the buffer
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int64_t p = s + j;
                        const uint32_t b = p < len ? at(p) : 0u;
                        v.w[j >> 2] |= b << (8 * (j & 3));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[4 * c + j] = v.w[j];
        }
    }
    // MerDNA(str) of the first `lim` (<= k) bytes held in w: 2-bit codes up to the first non-ACGT byte, 'A'-padded to k.
    // Four bases per step: code = x ^ (x >> 1) with x = bits 1..2 of the letter (A,C,G,T -> 0,1,2,3); a byte is a base
    // iff the letter that code stands for equals the byte with its case bit cleared (v_perm_b32 as a 4-entry table).
    __device__ __forceinline__ u128 encode_words(const uint32_t w[16], int lim, int &nvalid) const {
        uint64_t hi = 0, lo = 0, inv = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t x0 = (w[i] >> 1) & 0x03030303u;
            const uint32_t x = x0 ^ ((x0 >> 1) & 0x01010101u);
            const uint32_t expect = __builtin_amdgcn_perm(0u, 0x54474341u, x);
            const uint32_t d = expect ^ (w[i] & 0xDFDFDFDFu);
            const uint32_t nz = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;     // 0x80 per byte that differs
            const uint32_t c8 = (x * 0x40100401u) >> 24;                                      // b0<<6 | b1<<4 | b2<<2 | b3
            const uint32_t n4 = (((nz >> 7) * 0x01020408u) >> 24) & 0xFu;                     // bit j = byte j is no base
            if (i < 8) hi |= (uint64_t)c8 << (56 - 8 * i);
            else lo |= (uint64_t)c8 << (56 - 8 * (i - 8));
            inv |= (uint64_t)n4 << (4 * i);
        }
        if (lim < 64) inv |= ~0ull << lim;
        const int t = inv ? (int)__builtin_ctzll(inv) : 64;
        nvalid = t;
        if (t == 0) return mk(0, 0);
        return shl(shr(mk(hi, lo), 128 - 2 * t), 2 * (k - t));
    }

    // qf[jf.MerDNA(seq[a:b]).get_canonical()] -- python slice semantics, per lane
    __device__ __forceinline__ uint32_t cnt_seq(int64_t a, int64_t b) {
        int64_t lo, hi;
        guard(a, b);
        pyslice(len, a, b, lo, hi);
        const int n = (int)(hi - lo < k ? hi - lo : k);
        uint32_t w[16];
        load_window(lo, n, w);
        int nv;
        const u128 m = encode_words(w, n, nv);
        return clamp32(table_get(T, mix(canonical(m, k), T.B)));
    }
    // same for a string in LDS / global scratch: all byte loads are issued before the first is used (the loop that stops at
    // the first non-ACGT byte made every load wait for the previous one)
    __device__ __forceinline__ uint32_t cnt_str(const uint8_t *p, int n) const {
        const int lim = n < k ? n : k;
        uint32_t w[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            uint32_t v = 0;
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int q = 4 * x + y;
                const uint32_t b = q < lim ? (uint32_t)p[q] : 0u;
                v |= b << (8 * y);
            }
            w[x] = v;
        }
        int nv;
        const u128 m = encode_words(w, lim, nv);
        return clamp32(table_get(T, mix(canonical(m, k), T.B)));
    }

    // the same for a string given by a function q -> byte q (a trial string that is never materialised)
    template <typename F>
    __device__ __forceinline__ uint32_t cnt_fn(int n, F get) const {
        const int lim = n < k ? n : k;
        uint32_t w[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            uint32_t v = 0;
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int q = 4 * x + y;
                const uint32_t b = q < lim ? (uint32_t)get(q) : 0u;
                v |= b << (8 * y);
            }
            w[x] = v;
        }
        int nv;
        const u128 m = encode_words(w, lim, nv);
        return clamp32(table_get(T, mix(canonical(m, k), T.B)));
    }

    // ---------------- gap buffer ----------------
    __device__ void move_gap(int64_t to) {
        if (to == gs) return;
        if (to > gs) {  // bytes [gs+glen, to+glen) slide down to [gs, to): ascending, loads of a step before its stores
            const int64_t n = to - gs;
            const uint8_t *src = buf + gs + glen;
            uint8_t *dst = buf + gs;
            int64_t off = 0;
            for (; off + 4096 <= n; off += 4096) {          // 64 lanes x 4 x 16 B per step
                U16 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const U16 *>(src + off + (u * 64 + lane) * 16);
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<U16 *>(dst + off + (u * 64 + lane) * 16) = v[u];
            }
            for (; off < n; off += 256) {
                uint8_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { int64_t q = off + u * 64 + lane; v[u] = q < n ? src[q] : 0; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { int64_t q = off + u * 64 + lane; if (q < n) dst[q] = v[u]; }
            }
        } else {        // bytes [to, gs) slide up to [to+glen, gs+glen): descending from the top
            const int64_t n = gs - to;
            const uint8_t *src_end = buf + gs;               // one past the last source byte
            uint8_t *dst_end = buf + gs + glen;
            int64_t off = 0;                                 // bytes already moved, counted from the top
            for (; off + 4096 <= n; off += 4096) {
                U16 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const U16 *>(src_end - off - (u * 64 + lane + 1) * 16);
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<U16 *>(dst_end - off - (u * 64 + lane + 1) * 16) = v[u];
            }
            for (; off < n; off += 256) {
                uint8_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { int64_t q = off + u * 64 + lane; v[u] = q < n ? src_end[-1 - q] : 0; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { int64_t q = off + u * 64 + lane; if (q < n) dst_end[-1 - q] = v[u]; }
            }
        }
        gs = to;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    // seq = seq[:a] + patch + seq[b:]   (0 <= a <= b <= len), patch readable by every lane
    __device__ void replace(int64_t a, int64_t b, const uint8_t *patch, int64_t plen) {
        const uint64_t tr0 = phase_clock();
        replace_(a, b, patch, plen);
        tk[3] += phase_clock() - tr0;
    }
    __device__ void replace_(int64_t a, int64_t b, const uint8_t *patch, int64_t plen) {
        move_gap(a);
        glen += (b - a);
        if (glen < plen) { status = PS_GAP_EXHAUSTED; return; }
        if (nedit >= C->edit_cap) { status = PS_REC_OVERFLOW; return; }
        if (lane == 0) {
            EditRec e;
            e.a = a; e.plen = (int32_t)plen; e.oldlen = (int32_t)(b - a);
            C->edits[nedit] = e;
        }
        nedit++;
        for (int64_t q = lane; q < plen; q += 64) buf[gs + q] = patch[q];
        gs += plen;
        glen -= plen;
        len += plen - (b - a);
        delta += plen - (b - a);
        dirty_end = a + plen;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }

    // ---------------- LDS string helpers (lane-parallel copies, then a wave barrier) ----------------
    __device__ __forceinline__ void cp_seq(uint8_t *dst, int64_t lo, int64_t hi) {
        guard(lo, hi);
        for (int64_t q = lane; q < hi - lo; q += 64) dst[q] = at(lo + q);
    }
    __device__ __forceinline__ void cp_mem(uint8_t *dst, const uint8_t *src, int n) const {
        for (int q = lane; q < n; q += 64) dst[q] = src[q];
    }
    __device__ __forceinline__ void put(uint8_t *dst, uint8_t c) const { if (lane == 0) *dst = c; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }

    // ---------------- src/jasper.py:585-599 check_sequence ----------------
    // samples: trial[:k], trial[-k:], trial[i:i+k] for i in range(step, len-k, step); all must be >= thr
    __device__ bool check_sequence(const uint8_t *t, int n, uint32_t thr) {
        const int nmid = (n - k > step) ? (n - k - step + step - 1) / step : 0;  // len(range(step, n-k, step))
        const int jobs = 2 + nmid;
        bool ok = true;
        for (int base = 0; base < jobs; base += 64) {
            const int j = base + lane;
            bool bad = false;
            if (j < jobs) {
                uint32_t c;
                if (j == 0) c = cnt_str(t, n < k ? n : k);
                else if (j == 1) { int lo = n > k ? n - k : 0; c = cnt_str(t + lo, n - lo); }
                else { int i = step * (j - 1); c = cnt_str(t + i, k); }
                bad = c < thr;
            }
            if (__ballot(bad)) ok = false;
        }
        nlook += (uint64_t)jobs;
        return ok;
    }
    // number of windows of t (all n-k+1 of them) whose count is below thr
    __device__ int dense_bad(const uint8_t *t, int n, uint32_t thr) {
        int bad = 0;
        const int nw = n - k + 1;
        for (int base = 0; base < nw; base += 64) {
            const int i = base + lane;
            bool b = false;
            if (i < nw) b = cnt_str(t + i, k) < thr;
            bad += __popcll(__ballot(b));
        }
        if (nw > 0) nlook += (uint64_t)nw;
        return bad;
    }

    // ---------------- fix records ----------------
    __device__ void emit(uint8_t kind, int64_t index, uint8_t newc, uint8_t oldc, uint32_t rep, uint32_t aux_off, uint32_t aux_len) {
        if (nrec >= C->rec_cap) { status = PS_REC_OVERFLOW; return; }
        if (lane == 0) {
            FixRec r;
            r.index = index; r.chunk = chunk_id; r.seqno = seqno; r.pass = (uint8_t)pass; r.kind = kind;
            r.newc = newc; r.oldc = oldc; r.rep = rep; r.aux_off = aux_off; r.aux_len = aux_len;
            C->recs[nrec] = r;
        }
        nrec++;
        seqno++;
    }

    // ---------------- repairs (src/jasper.py:392-524). tbf = to_be_fixed in s_tbf, length L. Output in s_t1. --------
    // fix_k_case_sub :392-406
    __device__ uint8_t fix_k_case_sub(int L, uint32_t thr, int &outlen) {
        const uint8_t bad = s_tbf[k - 1];
        const char *order = "ACTG";
        for (int b = 0; b < 4; ++b) {
            if ((uint8_t)order[b] == bad) continue;
            cp_mem(s_t1, s_tbf, L);
            sync();
            put(s_t1 + k - 1, (uint8_t)order[b]);
            sync();
            if (check_sequence(s_t1, L, thr)) { outlen = L; return (uint8_t)order[b]; }
            sync();
        }
        return 0;
    }
    // fix_insert :409-419
    __device__ uint8_t fix_insert(int L, uint32_t thr, int &outlen) {
        cp_mem(s_t1, s_tbf, k - 1);
        cp_mem(s_t1 + k - 1, s_tbf + k, L - k);
        sync();
        if (check_sequence(s_t1, L - 1, thr)) { outlen = L - 1; return s_tbf[k - 1]; }
        sync();
        return 0;
    }
    // fix_del :422-431
    __device__ uint8_t fix_del(int L, uint32_t thr, int &outlen) {
        const char *order = "ATCG";
        for (int a = 0; a < 4; ++a) {
            cp_mem(s_t1, s_tbf, k - 1);
            cp_mem(s_t1 + k, s_tbf + k - 1, L - (k - 1));
            put(s_t1 + k - 1, (uint8_t)order[a]);
            sync();
            if (check_sequence(s_t1, L + 1, thr)) { outlen = L + 1; return (uint8_t)order[a]; }
            sync();
        }
        return 0;
    }
    // fixdiploid :340-382. returns 0, 's' or 'e'
    __device__ uint8_t fixdiploid(int L, uint32_t thr, int64_t gb, int64_t ga, uint8_t &left, uint8_t &right, int &outlen) {
        const uint8_t left_bad = s_tbf[L - k], right_bad = s_tbf[k - 1];
        int64_t gbsi = gb - k + 1; if (gbsi < 0) gbsi = 0;
        const int64_t h = (int64_t)((double)(k - 1 - L + k) / 2.0);
        int64_t alo, ahi, blo, bhi;
        if (ga + k - 1 + h < len) pyslice(len, ga + k - 1, ga + k - 1 + h, alo, ahi);
        else {
            if (!is_last) spec_fail = 1;   // only the true chunk end may take this branch
            int64_t st = ga + k - 1; if (st > len - 1) st = len - 1; pyslice(len, st, len, alo, ahi);
        }
        const int64_t before_len = ahi - alo;
        int64_t bs = gbsi - before_len + 1; if (bs < 0) bs = 0;
        pyslice(len, bs, gbsi + 1, blo, bhi);
        const int nb = (int)(bhi - blo), na = (int)(ahi - alo);
        if (nb + L + na > SMAX) { status = PS_STRING_TOO_LONG; return 0; }
        const char *order = "ACTG";
        for (int xi = 0; xi < 4; ++xi)
            for (int yi = 0; yi < 4; ++yi) {
                const uint8_t x = (uint8_t)order[xi], y = (uint8_t)order[yi];
                if (x == left_bad && y == right_bad) continue;
                if (x != left_bad && y != right_bad) continue;
                // trial = tbf[:L-k] + x + tbf[L-k+1:k-1] + y + tbf[k:]   (python slices; L-k+1 <= k-1 here)
                int n = 0;
                int64_t a0, a1;
                pyslice(L, 0, L - k, a0, a1); cp_mem(s_t1 + n, s_tbf + a0, (int)(a1 - a0)); n += (int)(a1 - a0);
                put(s_t1 + n, x); n += 1;
                pyslice(L, L - k + 1, k - 1, a0, a1); cp_mem(s_t1 + n, s_tbf + a0, (int)(a1 - a0)); n += (int)(a1 - a0);
                put(s_t1 + n, y); n += 1;
                pyslice(L, k, L, a0, a1); cp_mem(s_t1 + n, s_tbf + a0, (int)(a1 - a0)); n += (int)(a1 - a0);
                sync();
                cp_seq(s_t2, blo, bhi);
                cp_mem(s_t2 + nb, s_t1, n);
                cp_seq(s_t2 + nb + n, alo, ahi);
                sync();
                const bool ok = check_sequence(s_t2, nb + n + na, thr);
                sync();
                if (ok) { left = x; right = y; outlen = n; return (x == left_bad) ? (uint8_t)'e' : (uint8_t)'s'; }
            }
        return 0;
    }
    // fix_same_base_del :434-477. returns true; ridx, rbase, rrep; output in s_t1
    __device__ bool fix_same_base_del(int L, uint32_t thr, int &ridx, uint8_t &rbase, int &rrep, int &outlen) {
        if (thr > solid) return false;
        const uint8_t sb = s_tbf[k - 2];
        int inserted = 0;
        const int original_bad = L - k + 1;
        int current_bad = original_bad;
        const int max_ins = original_bad;
        if (L + max_ins > SMAX) { status = PS_STRING_TOO_LONG; return false; }
        while (inserted < max_ins) {
            // trial = tbf[:k-1] + sb*(inserted+1) + tbf[k-1:]
            inserted++;
            const int n = L + inserted;
            cp_mem(s_t1, s_tbf, k - 1);
            for (int q = lane; q < inserted; q += 64) s_t1[k - 1 + q] = sb;
            cp_mem(s_t1 + k - 1 + inserted, s_tbf + k - 1, L - (k - 1));
            sync();
            const int new_bad = dense_bad(s_t1, n, thr);
            sync();
            if (new_bad == 0) { ridx = k - 1; rbase = sb; rrep = inserted; outlen = n; return true; }
            if (new_bad >= current_bad) break;
            current_bad = new_bad;
        }
        const char *order = "ATCG";
        for (int a = 0; a < 4; ++a) {
            cp_mem(s_t1, s_tbf, k - 2);
            put(s_t1 + k - 2, (uint8_t)order[a]);
            cp_mem(s_t1 + k - 1, s_tbf + k - 2, L - (k - 2));
            sync();
            const bool ok = check_sequence(s_t1, L + 1, thr);
            sync();
            if (ok) { ridx = k - 2; rbase = (uint8_t)order[a]; rrep = 1; outlen = L + 1; return true; }
        }
        return false;
    }
    // fix_same_base_insertion :479-524
    __device__ bool fix_same_base_insertion(int L, uint32_t thr, int &ridx, uint8_t &rbase, int &rrep, int &outlen) {
        if (thr > solid) return false;
        const uint8_t sb = s_tbf[k - 1];
        int deleted = 0;
        const int original_bad = L - k + 1;
        int current_bad = original_bad;
        const int max_del = original_bad;
        while (deleted < max_del) {  // (tbf[k-1] == sb is always true, :494)
            current_bad -= 1;
            deleted += 1;
            // local = tbf[:k-1] + tbf[k-1+deleted:]
            const int n = L - deleted;
            if (n < k - 1) break;
            cp_mem(s_t1, s_tbf, k - 1);
            cp_mem(s_t1 + k - 1, s_tbf + k - 1 + deleted, n - (k - 1));
            sync();
            if (n == k) { sync(); break; }
            const int new_bad = dense_bad(s_t1, n, thr);
            sync();
            if (new_bad == 0) { ridx = k - 1; rbase = sb; rrep = deleted; outlen = n; return true; }
            if (new_bad >= current_bad) break;
            current_bad = new_bad;
        }
        // trials "tbf without its character i", i = L-k .. L-2, first one whose check_sequence samples are all solid (:507-520).
        // The trials are independent: several are evaluated per round, (trial, sample) per lane, straight from tbf; the
        // winner -- the FIRST passing i, as in the sequential loop -- is then written out.  (This loop was the slowest
        // thing a segment could meet: up to k-1 rounds of dependent lookups.)
        {
            const int n1 = L - 1;
            const int nmid = (n1 - k > step) ? (n1 - k - step + step - 1) / step : 0;     // len(range(step, n1-k, step))
            const int jobs = 2 + nmid;
            const int i_first = L - k > 0 ? L - k : 0;
            if (jobs <= 64) {
                const int tpr = 64 / jobs;                                           // trials per round
                for (int i0 = i_first; i0 < L - 1; i0 += tpr) {
                    const int ti = lane / jobs, j = lane - ti * jobs, i = i0 + ti;
                    const bool active = ti < tpr && i < L - 1;
                    bool bad = false;
                    if (active) {
                        int p, len;
                        if (j == 0) { p = 0; len = n1 < k ? n1 : k; }
                        else if (j == 1) { p = n1 > k ? n1 - k : 0; len = n1 - p; }
                        else { p = step * (j - 1); len = k; }
                        const uint32_t c = cnt_fn(len, [&](int q) { const int sidx = p + q; return s_tbf[sidx < i ? sidx : sidx + 1]; });
                        bad = c < thr;
                    }
                    const uint64_t mb = __ballot(active && bad);
                    for (int tt = 0; tt < tpr && i0 + tt < L - 1; ++tt) {
                        const uint64_t lanes = (jobs == 64 ? ~0ull : ((1ull << jobs) - 1ull)) << (tt * jobs);
                        nlook += (uint64_t)jobs;
                        if ((mb & lanes) == 0ull) {
                            const int iw = i0 + tt;
                            cp_mem(s_t1, s_tbf, iw);
                            cp_mem(s_t1 + iw, s_tbf + iw + 1, L - iw - 1);
                            sync();
                            ridx = iw; rbase = s_tbf[iw]; rrep = 1; outlen = L - 1;
                            return true;
                        }
                    }
                }
                return false;
            }
        }
        for (int i = L - k; i < L - 1; ++i) {
            if (i < 0) continue;
            cp_mem(s_t1, s_tbf, i);
            cp_mem(s_t1 + i, s_tbf + i + 1, L - i - 1);
            sync();
            const bool ok = check_sequence(s_t1, L - 1, thr);
            sync();
            if (ok) { ridx = i; rbase = s_tbf[i]; rrep = 1; outlen = L - 1; return true; }
        }
        return false;
    }

    // ---------------- src/jasper.py:527-583 base_extension ----------------
    // gkb / gka in s_gkb / s_gka (lengths nb, na). Returns patch length (patch in bfs_patch, slot kept until
    // release_scratch()) or -1 for None.
    __device__ int64_t base_extension(int64_t Ltbf, int nb, int na, uint32_t thr) {
        if (nb < k || na < k || thr > solid) return -1;
        // take a scratch slot (searches are rare; a wave holds a slot only while it searches and splices)
        uint32_t slot = (uint32_t)((blockIdx.x * 2654435761u) % pool.nslots);
        for (;;) {
            unsigned int old = 1;
            if (lane == 0) old = atomicCAS(&pool.locks[slot], 0u, 1u);
            old = __shfl(old, 0);
            if (old == 0u) break;
            slot = (slot + 1) % pool.nslots;
            __builtin_amdgcn_s_sleep(16);
        }
        bfs_slot = (int)slot;
        // (the slot's last user may have run on another CU: nothing of its bytes that this CU's L1 still holds may be read)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        uint8_t *sb = pool.base + (size_t)slot * pool.stride;
        bfs_nodes = reinterpret_cast<uint32_t *>(sb);
        bfs_front = sb + pool.off_front;
        bfs_patch = sb + pool.off_patch;
        const int64_t r = base_extension_impl(Ltbf, thr);
        if (r < 0) release_scratch();
        return r;
    }
    __device__ void release_scratch() {
        if (bfs_slot < 0) return;
        // Every store of this wave into the slot must have ARRIVED before the slot is given up: a workgroup-scope fence does not
        // wait for that, and a store still on its way landed in the arrays of the slot's next user (another CU) now and then --
        // found as a path search that returned different patches from run to run once slots were few and the memory busy
        // (several lanes, 64 slots; 16 slots: 118 of 150 runs).  Searches are rare: the agent-scope release costs nothing.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) atomicExch(&pool.locks[bfs_slot], 0u);
        bfs_slot = -1;
    }
    __device__ int64_t base_extension_impl(int64_t Ltbf, uint32_t thr) {
        const int64_t min_overlap = 5, slack = 10;
        const int64_t max_ext = pyround((double)(Ltbf - 2 * k) * 1.2) + min_overlap + slack;
        const int64_t min_patch_len = pyround((double)(Ltbf - 2 * k) / 1.2) - slack;
        FrontEntry *F = reinterpret_cast<FrontEntry *>(bfs_front);
        const uint32_t fcap = pool.front_cap;
        uint32_t *nodes = bfs_nodes;
        uint32_t nn = 1;            // node 0 = the initial one-base path (last base of the good k-mer before)
        uint32_t np = 1;
        const int TCAP = k + 3;
        if (lane == 0) {
            nodes[0] = 0;
            F[0].node = 0; F[0].tlen = (uint16_t)k; F[0].alive = 1; F[0].pad = 0;
        }
        for (int q = lane; q < k; q += 64) F[0].tail[q] = s_gkb[q];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        const int glo = (k > 5) ? 5 : (k == 5 ? 0 : 5 - k);   // good_k_mer_after[-(k-5):]
        for (int64_t i = 1; i < max_ext; ++i) {
            // paths = [l for l in paths if len(l) > 0]   (:542) -- order-preserving in-place compaction
            uint32_t w = 0;
            for (uint32_t base = 0; base < np; base += 64) {
                const uint32_t e = base + lane;
                FrontEntry fe;
                bool alive = false;
                if (e < np) { fe = F[e]; alive = fe.alive != 0; }
                const uint64_t m = __ballot(alive);
                const uint32_t dst = w + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (alive && dst != e) F[dst] = fe;
                w += (uint32_t)__popcll(m);
            }
            np = w;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            if (np > 5000) return -1;                                            // :543-546
            if (np == 0) return -1;  // nothing left: the python loop just spins to max_ext and returns None
            const uint32_t last_path = np;
            for (uint32_t g = 0; g < last_path; g += 16) {
                // 16 paths x 4 bases per round: score = qf[km1 + bases[j]]     (:551-554)
                const uint32_t pp = g + (uint32_t)(lane >> 2);
                const int jj = lane & 3;
                uint32_t score = 0;
                if (pp < last_path) {
                    const FrontEntry *fe = &F[pp];
                    const int tl = fe->tlen;
                    const uint8_t bj = (uint8_t)("ACGT"[jj]);
                    // km1 + base: the last k-1 tail bytes with four 16-B loads in flight (tl <= k+3, so the 64 bytes read
                    // from tail + tl-(k-1) end inside tail[72]), then the candidate base as byte k-1
                    uint32_t w[16];
                    const uint8_t *src = fe->tail + (tl - (k - 1));
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const U16 v = *reinterpret_cast<const U16 *>(src + 16 * c4);
                        w[4 * c4] = v.w[0]; w[4 * c4 + 1] = v.w[1]; w[4 * c4 + 2] = v.w[2]; w[4 * c4 + 3] = v.w[3];
                    }
                    {
                        const int bi = k - 1;
#pragma unroll
                        for (int x = 0; x < 16; ++x)
                            if (x == (bi >> 2)) w[x] = (w[x] & ~(0xFFu << (8 * (bi & 3)))) | ((uint32_t)bj << (8 * (bi & 3)));
                    }
                    int nv;
                    const u128 m = encode_words(w, k, nv);
                    score = clamp32(table_get(T, mix(canonical(m, k), T.B)));
                }
                const uint32_t gend = (last_path - g) < 16u ? (last_path - g) : 16u;
                nlook += 4ull * gend;
                for (uint32_t q = 0; q < gend; ++q) {
                    const uint32_t p = g + q;
                    int ext = -1;                      // first base that extended this path
                    const uint32_t pnode = F[p].node;  // uniform loads
                    const int tl = F[p].tlen;
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t sc = __shfl(score, (int)(q * 4 + j));
                        if (sc < thr) continue;
                        const uint8_t bj = (uint8_t)("ACGT"[j]);
                        if (i >= min_overlap && i >= min_patch_len) {           // :557
                            // last_bases[-5:] == good_k_mer_after[0:5]         (:558) ; last_bases = km1 + base
                            struct __attribute__((packed, aligned(1))) U4 { uint32_t v; };
                            const uint32_t last4 = reinterpret_cast<const U4 *>(F[p].tail + (tl - 4))->v;
                            const uint32_t want4 = (uint32_t)s_gka[0] | ((uint32_t)s_gka[1] << 8) | ((uint32_t)s_gka[2] << 16) | ((uint32_t)s_gka[3] << 24);
                            const bool same = last4 == want4 && bj == s_gka[4];
                            if (same) {
                                // path_connected = (start_km1 + path_before + base + gka[-(k-5):])[-(2k-1):]  (:560/:563)
                                int n = 0;
                                const int take = tl < TCAP ? tl : TCAP;
                                cp_mem(s_t1, F[p].tail + (tl - take), take); n += take;
                                put(s_t1 + n, bj); n += 1;
                                cp_mem(s_t1 + n, s_gka + glo, k - glo); n += k - glo;
                                sync();
                                const int off = n > 2 * k - 1 ? n - (2 * k - 1) : 0;
                                const bool ok = check_sequence(s_t1 + off, n - off, thr);   // :567
                                sync();
                                if (ok) {
                                    if (i == min_overlap) return -1;                          // :568-571 "patch empty"
                                    // return_path = (path_before + base)[1:-5]  = path_before[1 : i-4]   (:561/:564)
                                    const int64_t plen = i - 5;
                                    if (plen > (int64_t)pool.patch_cap) { status = PS_BFS_ARENA; return -1; }
                                    if (lane == 0) {
                                        uint32_t nd = pnode;
                                        for (int u = 0; u < 4; ++u) nd = nodes[nd] >> 2;          // drop path[i-1..i-4]
                                        for (int64_t u = plen - 1; u >= 0; --u) {
                                            bfs_patch[u] = (uint8_t)("ACGT"[nodes[nd] & 3u]);
                                            nd = nodes[nd] >> 2;
                                        }
                                    }
                                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                                    return plen;
                                }
                            }
                        }
                        if (ext < 0) {
                            ext = j;                                                          // :576-578 (applied below)
                        } else {                                                              // :579-580 sibling
                            if (np >= fcap || nn >= pool.node_cap) { status = PS_BFS_ARENA; return -1; }
                            if (lane == 0) nodes[nn] = (pnode << 2) | (uint32_t)j;
                            // sibling tail = tail_before + base
                            const int keep = tl < TCAP ? tl : TCAP - 1;
                            for (int u = lane; u < keep; u += 64) F[np].tail[u] = F[p].tail[tl - keep + u];
                            if (lane == 0) {
                                F[np].tail[keep] = bj;
                                F[np].tlen = (uint16_t)(keep + 1); F[np].node = nn; F[np].alive = 1; F[np].pad = 0;
                            }
                            nn++; np++;
                        }
                    }
                    // apply the first extension to the path itself, or kill it                (:576-578,:581-582)
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    if (ext >= 0) {
                        if (nn >= pool.node_cap) { status = PS_BFS_ARENA; return -1; }
                        const uint8_t bj = (uint8_t)("ACGT"[ext]);
                        if (lane == 0) nodes[nn] = (pnode << 2) | (uint32_t)ext;
                        if (tl < TCAP) {
                            if (lane == 0) { F[p].tail[tl] = bj; F[p].tlen = (uint16_t)(tl + 1); F[p].node = nn; }
                        } else {
                            uint8_t v = 0;
                            if (lane < TCAP - 1) v = F[p].tail[lane + 1];   // k+3 <= 67 > 64 lanes only when k > 61
                            uint8_t v2 = 0;
                            if (lane + 64 < TCAP - 1) v2 = F[p].tail[lane + 65];
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                            if (lane < TCAP - 1) F[p].tail[lane] = v;
                            if (lane + 64 < TCAP - 1) F[p].tail[lane + 64] = v2;
                            if (lane == 0) { F[p].tail[TCAP - 1] = bj; F[p].node = nn; }
                        }
                        nn++;
                    } else if (lane == 0) {
                        F[p].alive = 0;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            }
        }
        return -1;
    }

    // ---------------- src/jasper.py:226-332 fixing_sid ----------------
    // tbf in s_tbf (only when n <= k), L = len(to_be_fixed). Emits records, splices the chunk.
    template <typename F>
    __device__ __forceinline__ auto timed(int slot, F f) -> decltype(f()) {
        const uint64_t t0 = phase_clock();
        auto r = f();
        tk[slot] += phase_clock() - t0;
        return r;
    }
    __device__ void fixing_sid(int64_t L64, uint32_t thr, int64_t n, int64_t gb, int64_t ga) {
        int64_t s0 = gb - k + 2; if (s0 < 0) s0 = 0;
        const int L = (int)L64;
        int outlen = 0;
        if (n == k) {                                                          // :232
            uint8_t b = timed(4, [&]() { return fix_k_case_sub(L, thr, outlen); });
            if (b) {
                emit('s', ga - 1, b, at(ga - 1), 1, 0, 0);                    // :235-237
                replace(s0, ga + k - 1, s_t1, outlen);                        // :238
            } else {
                b = timed(5, [&]() { return fix_insert(L, thr, outlen); });
                if (b) {
                    emit('i', ga - 1, '-', at(ga - 1), 1, 0, 0);              // :242-244
                    replace(s0, ga + k - 1, s_t1, outlen);
                }
            }
        } else if (n == k - 1) {                                               // :247
            uint8_t b = timed(6, [&]() { return fix_del(L, thr, outlen); });
            if (b) {
                emit('d', ga, b, '-', 1, 0, 0);                               // :250-253
                replace(s0, ga + k - 1, s_t1, outlen);
            } else {
                uint8_t left = 0, right = 0;
                const uint8_t lr = timed(7, [&]() { return fixdiploid(L, thr, gb, ga, left, right, outlen); });
                if (lr) {
                    if (lr == 's') emit('s', ga - 1, left, at(ga - 1), 1, 0, 0);   // :257-260
                    else emit('s', gb + 1, right, at(gb + 1), 1, 0, 0);            // :262-264
                    replace(s0, ga + k - 1, s_t1, outlen);
                } else if (status == PS_OK) {
                    int idx = 0, rep = 0; uint8_t bs = 0;
                    if (timed(9, [&]() { return fix_same_base_insertion(L, thr, idx, bs, rep, outlen); })) {    // :267-272
                        emit('i', idx + s0, '-', bs, (uint32_t)rep, 0, 0);
                        replace(s0, ga + k - 1, s_t1, outlen);
                    }
                }
            }
        } else if (n < k - 1 && n > 1 && L64 >= k) {                           // :274
            int idx = 0, rep = 0; uint8_t bs = 0;
            if (timed(8, [&]() { return fix_same_base_del(L, thr, idx, bs, rep, outlen); })) {             // :275-280
                emit('d', idx + s0, bs, '-', (uint32_t)rep, 0, 0);
                replace(s0, ga + k - 1, s_t1, outlen);
            } else if (status == PS_OK) {
                uint8_t left = 0, right = 0;
                const uint8_t lr = timed(7, [&]() { return fixdiploid(L, thr, gb, ga, left, right, outlen); });
                if (lr) {
                    if (lr == 's') emit('s', ga - 1, left, at(ga - 1), 1, 0, 0);
                    else emit('s', gb + 1, right, at(gb + 1), 1, 0, 0);
                    replace(s0, ga + k - 1, s_t1, outlen);
                } else if (status == PS_OK && timed(9, [&]() { return fix_same_base_insertion(L, thr, idx, bs, rep, outlen); })) {  // :294-299
                    emit('i', idx + s0, '-', bs, (uint32_t)rep, 0, 0);
                    replace(s0, ga + k - 1, s_t1, outlen);
                }
            }
        } else if (n > k) {                                                    // :301
            int64_t blo, bhi, alo, ahi;
            guard(gb - k + 1, gb + 1);
            guard(ga, ga + k);
            pyslice(len, gb - k + 1, gb + 1, blo, bhi);                        // :302
            pyslice(len, ga, ga + k, alo, ahi);                                // :303
            cp_seq(s_gkb, blo, bhi);
            cp_seq(s_gka, alo, ahi);
            sync();
            const int64_t plen = timed(10, [&]() { return base_extension(L64, (int)(bhi - blo), (int)(ahi - alo), thr); });
            sync();
            if (plen >= 0 && status == PS_OK) {
                // record: patch ++ original segment seq[gb+1:ga]; the host aligns them (src/jasper.py:309-329)
                int64_t olo, ohi;
                pyslice(len, gb + 1, ga, olo, ohi);
                const int64_t on = ohi - olo;
                if ((uint64_t)naux + (uint64_t)plen + (uint64_t)on > (uint64_t)C->aux_cap) { status = PS_AUX_OVERFLOW; release_scratch(); return; }
                for (int64_t q = lane; q < plen; q += 64) C->aux[naux + q] = bfs_patch[q];
                for (int64_t q = lane; q < on; q += 64) C->aux[naux + plen + q] = at(olo + q);
                emit('x', gb + 1, 0, 0, (uint32_t)on, naux, (uint32_t)plen);
                naux += (uint32_t)(plen + on);
                replace(gb + 1, ga, bfs_patch, plen);                          // :312
            }
            release_scratch();
        }
    }

    // ---------------- src/jasper.py:150-223 handle_bad_kmers ----------------
    __device__ int64_t handle_bad_kmers(int64_t i, int64_t &wrong, bool fix, int64_t rolling_thre, bool &brk) {
        brk = false;
        const uint64_t th0 = phase_clock();
        uint32_t thre = solid;
        if (rolling_thre > 0) thre = (uint32_t)rolling_thre;                   // :151-153
        // backward: j = i-1; while cnt(seq[j:j+k]) < thre and j >= 0: j -= 1      (:155-159), 64 candidates per round
        int64_t j = i - 1;
        for (;;) {
            const int64_t jl = j - lane;
            bool stop = true, oob = false;
            if (!is_first && jl < glo) oob = true;                 // left of what this segment may assume
            else if (jl >= 0) stop = !(cnt_seq(jl, jl + k) < thre);
            // jl == -1 stops the loop whatever the count; jl < -1 is never reached
            const uint64_t m = __ballot(stop);
            nlook += 64;
            if (m) {
                const int f = (int)__builtin_ctzll(m);
                if (__shfl((int)oob, f)) spec_fail = 1;
                j = j - (int64_t)f;
                break;
            }
            j -= 64;
        }
        if (j < -1) j = -1;
        int64_t gb = j + k - 1;                                                // :160
        uint32_t prev = cnt_seq(j, k + j);                                     // :161
        if (j == -1) gb = -1;                                                  // :164
        // forward (:167-178)
        for (;;) {
            const int64_t il = i + lane;
            bool cont = false;
            if (il < len - k + 1) cont = cnt_seq(il, il + k) < thre;
            const bool giveup = cont && rolling_thre != 0 && (il - j > k);     // :173-176
            const uint64_t m = __ballot(!cont || giveup);
            nlook += 64;
            if (m) {
                const int f = (int)__builtin_ctzll(m);
                const bool g = __shfl((int)giveup, f) != 0;
                i += f;
                if (!is_last && i >= len - k + 1) spec_fail = 1;
                if (g) return i + 1;
                break;
            }
            i += 64;
        }
        int64_t ga = i;                                                        // :179
        nlook += 4;
        if (2ull * cnt_seq(gb - k + 2, gb + 2) < (uint64_t)solid && 2ull * cnt_seq(gb - k + 3, gb + 3) < (uint64_t)solid) {
            // too_low_flag only (:182-183)
        } else if (rolling_thre == 0) {                                        // :184
            while (2ull * cnt_seq(gb - k + 2, gb + 2) >= (uint64_t)prev && gb - k + 1 < ga) {   // :185
                if (gb == -1) break;
                if (2ull * prev >= (uint64_t)thre && 2ull * cnt_seq(gb - k + 2, gb + 2) < (uint64_t)thre &&
                    2ull * cnt_seq(gb - k + 3, gb + 3) < (uint64_t)thre) break;                  // :188-190
                prev = cnt_seq(gb - k + 2, gb + 2);                            // :192
                gb++;
                nlook += 4;
            }
            if (gb >= len - 1) { if (!is_last) spec_fail = 1; brk = true; return i; }   // :194-195
        }
        int64_t s0 = gb - k + 2; if (s0 < 0) s0 = 0;
        if (s0 + k + k >= len) { if (!is_last) spec_fail = 1; brk = true; return s0 + k + k; }   // :197-198
        {
            // four independent lookups (:199-205), one per lane
            uint32_t c = 0;
            if (lane == 0) c = cnt_seq(s0 + 1, s0 + k + 1);
            else if (lane == 1) c = cnt_seq(s0 + k - 2, s0 + k + k - 2);
            else if (lane == 2) c = cnt_seq(s0 + k - 1, s0 + k + k - 1);
            else if (lane == 3) c = cnt_seq(s0 + k, s0 + k + k);
            const uint64_t lowm = __ballot(lane < 4 && c < thre) & 0xFull;
            nlook += 4;
            if (lowm == 0x7ull) ga = s0 + k;
        }
        int64_t tlo, thi;
        pyslice(len, s0, ga + k - 1, tlo, thi);                                // :206
        int64_t n = ga - s0; if (n < 0) n = 0;                                 // :207
        wrong += n;
        const uint64_t tf0 = phase_clock();
        tk[1] += tf0 - th0;
        struct FixTimer { uint64_t &acc; uint64_t t0; __device__ ~FixTimer() { acc += phase_clock() - t0; } } fix_timer{tk[2], tf0};
        if (fix) {
            if (gb < 0) return i;                                              // :211-212
            const int64_t L = thi - tlo;
            if (n <= k) {
                if (L > SMAX) { status = PS_STRING_TOO_LONG; return i; }
                cp_seq(s_tbf, tlo, thi);
                sync();
            }
            fixing_sid(L, thre, n, gb, ga);                                    // :213
            sync();
        }
        return i;                                                              // :223
    }

    // first position >= i on the stride i, i+(k-1), ... that is not a plain "good k-mer, i += k-1" step
    // (src/jasper.py:97,100), or a position >= len-k+1
    __device__ int64_t skip_good(int64_t i) {
        const int64_t end = len - k + 1;
        for (;;) {
            const int64_t p = i + (int64_t)lane * (k - 1);
            bool ev = true;
            bool known = false;
            if (p < end && cls != nullptr && p >= dirty_end + k) {
                const int64_t o = p - delta + seg_lo;              // pass-start chunk coordinate
                if (!is_last && o >= stop_orig) known = true;      // (ev stays true) the next segment's: hand over here
                else if (o >= 0 && o < cls_n) { known = true; ev = cls[o] != PC_CLEAN; }
            }
            if (p < end && !known) {
                // one pass over the window: 2-bit encode + validity
                uint32_t w[16];
                load_window(p, k, w);
                int nv;
                const u128 m = encode_words(w, k, nv);
                const bool valid = nv == k;
                if (valid) {
                    const uint32_t occ = clamp32(table_get(T, mix(canonical(m, k), T.B)));
                    ev = occ < solid;
                    if (!ev && p > 0) {
                        const int64_t a = p - k > 0 ? p - k : 0;
                        const int64_t b = p > k ? p : k;
                        ev = 50ull * occ < (uint64_t)cnt_seq(a, b);            // :80
                    }
                }
            }
            const uint64_t mask = __ballot(ev);
            nlook += 128;
            if (mask) return i + (int64_t)__builtin_ctzll(mask) * (k - 1);
            i += 64ll * (k - 1);
        }
    }

    // ---------------- src/jasper.py:50-104, one chunk, one pass ----------------
    __device__ void walk(bool fix, int64_t start_i, int64_t &wrong_out, long long &arrive_out) {
        int64_t i = start_i, wrong = 0;
        bool handed_over = false;
        arrive_out = ARRIVE_FAIL;
        while (i < len - k + 1 && status == PS_OK) {                           // :55
            if (__ballot(spec_fail != 0)) { spec_fail = 1; break; }
            const uint64_t ts0 = phase_clock();
            i = skip_good(i);
            tk[0] += phase_clock() - ts0;
            if (i >= len - k + 1) { if (!is_last) spec_fail = 1; break; }
            // arriving at the next sync point: the next segment takes over from here
            if (!is_last && (i - delta + seg_lo) >= stop_orig) {
                if (i < dirty_end + k) spec_fail = 1;          // (never seen: boundaries lie >= 4k right of any event)
                else { handed_over = true; arrive_out = i - delta + seg_lo; }
                break;
            }
            // the reference's own loop body at position i
            uint8_t ch = 'A';
            if (lane < k) ch = at(i + lane);
            const uint64_t inwin = (k >= 64) ? ~0ull : ((1ull << k) - 1ull);
            const uint64_t mN = __ballot(ch == 'N') & inwin;                   // :57-60
            if (mN) {
                const int f = (int)__builtin_ctzll(mN);
                i += f + 1;
                if (f == 0) {  // a run of N: every further step is again "N at offset 0 -> i += 1"
                    for (;;) {
                        const int64_t q = i + lane;
                        const bool stop = !(q < len - k + 1 && at(q) == 'N');
                        const uint64_t m = __ballot(stop);
                        if (m) { i += (int64_t)__builtin_ctzll(m); break; }
                        i += 64;
                    }
                }
                continue;
            }
            const uint64_t mn = __ballot(ch == 'n') & inwin;                   // :61-64
            if (mn) { i += (int64_t)__builtin_ctzll(mn) + 1; continue; }
            const uint64_t mo = __ballot(code(ch) < 0) & inwin;                // :65-68
            if (mo) { i += 1; continue; }
            const uint32_t occ = cnt_seq(i, i + k);                            // :70-71
            nlook += 1;
            bool brk = false;
            if (occ < solid) {                                                 // :73
                i = handle_bad_kmers(i, wrong, fix, 0, brk);
                if (brk) break;
                continue;
            }
            bool cond2 = false;
            if (i > 0) {                                                       // :80
                const int64_t a = i - k > 0 ? i - k : 0;
                const int64_t b = i > k ? i : k;
                cond2 = 50ull * occ < (uint64_t)cnt_seq(a, b);
                nlook += 1;
            }
            if (!cond2) { i += k - 1; continue; }                              // :100
            // rolling mean of the counts sampled every `step` over the previous k positions (:82-89)
            int64_t ind0 = i - k > 0 ? i - k : 0;
            int64_t num = (i - ind0 + step - 1) / step;                        // iterations of `while ind < i`
            double sum = 0.0;
            for (int64_t base = 0; base < num; base += 64) {
                const int64_t t = base + lane;
                unsigned long long c = 0;
                if (t < num) { const int64_t ind = ind0 + (t + 1) * step; c = cnt_seq(ind, ind + k); }
                // exact integer sum across lanes
                for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
                sum += (double)c;
            }
            nlook += (uint64_t)num;
            const int64_t rolling = pyround(sum / (double)num / 50.0);        // :89
            if ((int64_t)occ < rolling) {                                      // :90
                i = handle_bad_kmers(i, wrong, fix, pyround(sum / (double)num / 2.0), brk);   // :93
                if (brk) break;
            } else {
                i += k - 1;                                                    // :97
            }
        }
        if (!is_last && !handed_over && status == PS_OK) spec_fail = 1;   // ran off the segment instead of reaching the sync point
        if (__ballot(spec_fail != 0)) spec_fail = 1;
        if (is_last && status == PS_OK && !spec_fail) arrive_out = ARRIVE_END;
        if (spec_fail || status != PS_OK) arrive_out = ARRIVE_FAIL;
        wrong_out = wrong;
    }
};

// The arrival slot is the ONLY thing a successor reads from its predecessor, so relaxed agent-scope atomics are enough
// (they go past the per-XCD L2).  Release/acquire here would write back / invalidate a whole L2 per hop: ~50 us each.
__device__ __forceinline__ void publish_arrival(long long *slot, long long v) {
    if (threadIdx.x == 0) __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (two waves per SIMD: the walk is one long state machine -- left alone the compiler spends 280 registers on it, ONE wave per SIMD,
//  1024 segments on the chip at a time, and pass 0 of a 47-Mb batch has 3824; capped at 256 registers the polish call takes 3.73
//  instead of 4.00 ms; at 168 or 128 registers what it spills costs what the third and fourth wave bring)
__global__ __launch_bounds__(64, 2) void seg_walk_kernel(TableDev T, SegDev *segs, int n_segs, PolishParams P, int pass, ScratchPool pool,
                                                      unsigned int *ticket) {
    __shared__ uint8_t s_tbf[SMAX], s_t1[SMAX], s_t2[SMAX], s_gkb[64], s_gka[64];
    // segments are taken in the order the waves START (a ticket, not blockIdx): a chained segment spins on its
    // predecessor's arrival, and a ticket guarantees that predecessor is already running or done
    unsigned int tk = 0;
    if (threadIdx.x == 0) tk = atomicAdd(ticket, 1u);
    const int c = (int)__shfl(tk, 0);
    if (c >= n_segs) return;
    SegDev *C = &segs[c];
    if (C->status != PS_OK) { publish_arrival(C->arrive, ARRIVE_FAIL); return; }
    if (!C->chain_in) publish_arrival(C->arrive, ARRIVE_WALKING);
    const int k = P.k;
    const int lane = threadIdx.x;
    const uint64_t t0 = wall_clock64();
    int64_t start_i = C->start_i;
    if (C->chain_in) {
        // (1) while the predecessor is still walking: can anything at all happen in my range?  Every window start the walk
        //     can visit here, [my boundary, the next boundary + k) or up to the chunk end, all CLEAN -> it only steps.
        const int64_t lo = C->seg_lo + 4ll * k;
        int64_t hi = C->last ? C->cls_n : C->stop_orig + k;
        if (hi > C->cls_n) hi = C->cls_n;
        bool dirty = C->cls == nullptr;
        static_assert(PC_CLEAN == 0, "the clean test below ORs class bytes");
        for (int64_t p0 = lo; p0 < hi && !dirty; p0 += 64 * 16) {
            bool nc = false;
            const int64_t p = p0 + (int64_t)lane * 16;
            if (p + 16 <= hi) {
                struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
                const V16 v = *reinterpret_cast<const V16 *>(C->cls + p);
                nc = (v.w[0] | v.w[1] | v.w[2] | v.w[3]) != 0u;
            } else {
                for (int q = 0; q < 16; ++q) nc = nc || (p + q < hi && C->cls[p + q] != PC_CLEAN);
            }
            dirty = __ballot(nc) != 0ull;
        }
        // (2) where does the walk arrive?  Segments are taken by ticket, so every predecessor is resident or done.  A segment says
        //     at once what it is: CLEAN (nothing can happen in its range: the walk only steps through it, so its arrival follows from
        //     ANY earlier arrival of the chain -- stepping by k - 1 from a to the first position >= stop and then on to a later stop
        //     is stepping from a to that later stop) or WALKING.  A clean segment therefore does not wait for its predecessor but
        //     looks back, 64 slots per load, past the clean ones to the nearest published arrival; the chain of dependent waits
        //     is as long as the chunk's DIRTY segments, not as all of them (47 Mb, passes 1 and 2: ~290 chained segments per chunk).
        if (lane == 0) __hip_atomic_store(C->arrive, dirty ? ARRIVE_WALKING : ARRIVE_CLEAN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long a = ARRIVE_FAIL;
        {
            // (bounded: a predecessor that never publishes -- which no code path allows -- must not hang the GPU; after ~2^24
            // polls, seconds, the segment gives up and the host redoes the chunk unsegmented)
            int back = 1;                                            // lane l looks at segment c - back - l
            for (uint32_t spins = 0;; ++spins) {
                const int idx = c - back - lane;
                long long v = ARRIVE_FAIL;
                if (idx >= 0) v = __hip_atomic_load(C->arrive - (c - idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool published = v >= 0 || v == ARRIVE_FAIL || v == ARRIVE_END;
                const bool skip = v == ARRIVE_CLEAN && !dirty;           // (a segment that walks needs its predecessor's own arrival)
                const unsigned long long stopper = __ballot(!skip);
                if (stopper) {
                    const int l = (int)__builtin_ctzll(stopper);
                    const bool ok = (__ballot(published) >> l) & 1ull;
                    if (ok) {
                        a = __shfl(v, l);
                        if (back + l > 1 && a >= 0) {                    // looked past clean segments: the arrival at MY boundary follows
                            const long long stop = segs[c - 1].stop_orig;
                            if (a < stop) a += ((stop - a + (k - 2)) / (k - 1)) * (long long)(k - 1);
                        }
                        break;
                    }
                    if (spins > (1u << 24)) { a = ARRIVE_FAIL; break; }
                    __builtin_amdgcn_s_sleep(4);                         // WALKING or not started yet: look again
                } else {
                    back += 64;                                          // 64 clean ones in a row: further back
                    if (spins > (1u << 24)) { a = ARRIVE_FAIL; break; }
                }
            }
        }
        if (a < 0 || a < lo || a - C->seg_lo >= C->len0) {       // the predecessor gave up, or an arrival I cannot take over
            if (lane == 0) { C->spec_fail = 1; C->ticks = wall_clock64() - t0; }
            publish_arrival(C->arrive, ARRIVE_FAIL);
            return;
        }
        if (!dirty) {
            const int64_t stop = C->last ? C->cls_n : C->stop_orig;
            const int64_t steps = a >= stop ? 0 : (stop - a + (k - 2)) / (k - 1);
            if (lane == 0) {
                C->took_shortcut = 1;
                C->lookups = 2ull * (uint64_t)steps;
                C->ticks = wall_clock64() - t0;
            }
            publish_arrival(C->arrive, C->last ? ARRIVE_END : a + steps * (k - 1));
            return;
        }
        start_i = a - C->seg_lo;
    }
    Walker w;
    w.T = T; w.k = P.k; w.step = P.step; w.lane = threadIdx.x; w.solid = P.solid;
    w.buf = C->buf; w.len = C->len; w.gs = C->gs; w.glen = C->glen; w.cap = C->cap;
    w.C = C; w.chunk_id = C->chunk; w.nrec = 0; w.naux = 0; w.seqno = 0; w.nedit = 0; w.pass = pass;
    w.status = PS_OK; w.nlook = 0; for (int q = 0; q < 12; ++q) w.tk[q] = 0;
    w.s_tbf = s_tbf; w.s_t1 = s_t1; w.s_t2 = s_t2; w.s_gkb = s_gkb; w.s_gka = s_gka;
    w.delta = 0; w.dirty_end = INT64_MIN / 2; w.glo = P.k;
    w.is_first = C->first != 0; w.is_last = C->last != 0; w.spec_fail = 0;
    w.cls = C->cls; w.cls_n = C->cls_n; w.seg_lo = C->seg_lo; w.stop_orig = C->stop_orig;
    w.pool = pool; w.bfs_slot = -1; w.bfs_nodes = nullptr; w.bfs_front = nullptr; w.bfs_patch = nullptr;
    const bool fix = P.fix && pass < P.passes;                                 // src/jasper.py:37-38
    int64_t wrong = 0;
    long long arrive = ARRIVE_FAIL;
    w.walk(fix, start_i, wrong, arrive);
    w.release_scratch();
    if (threadIdx.x == 0) {
        C->ticks = wall_clock64() - t0;
        for (int q = 0; q < 12; ++q) C->tk[q] = w.tk[q];
        C->len = w.len; C->gs = w.gs; C->glen = w.glen;
        C->nrec = w.nrec; C->naux = w.naux; C->nedit = w.nedit; C->status = w.status; C->spec_fail = w.spec_fail;
        C->wrong = wrong;
        C->lookups = w.nlook;
    }
    publish_arrival(C->arrive, arrive);
}

// ---------------------------------------------------------------------------------------------------------
// Dense scan (K4/K5): count of EVERY window of a contiguous text.  Same LDS staging and rolling recurrence as
// count_kernel (table.hip); a window that contains a non-ACGT byte gets valid = 0.
// ---------------------------------------------------------------------------------------------------------
constexpr int SC_THREADS = 256, SC_GROUP = 16, SC_TILE = SC_THREADS * SC_GROUP, SC_HALO = 4;

// ---- the kernels around the walk take their work as a flat list of (segment, 4 KiB piece): segments run from a few hundred bytes
// to a whole clean cell, and "blocks per segment" left a pass waiting for the blocks of its longest one.  The host knows every
// segment's pass-start lengths (make_pieces); what a walk added or removed falls to the segment's last piece.
__device__ __forceinline__ void piece_range(const SegPiece P, int64_t n, int64_t &q_lo, int64_t &q_hi) {
    q_lo = (int64_t)(P.piece & ~SEG_PIECE_LAST) * SEG_PIECE;
    q_hi = (P.piece & SEG_PIECE_LAST) ? n : q_lo + SEG_PIECE;
    if (q_hi > n) q_hi = n;
}

// copy each segment's text range out of its chunk into the segment's gap buffer (text right of the gap); and preset what the walk
// behind it and the next pass expect, instead of fills on the stream: the arrive slots (with the two guard slots), the walk's ticket,
// the candidate count (fetched by now) and the changed-text flags (read by now; the stitch sets them again)
__global__ __launch_bounds__(256) void seg_init_kernel(const SegDev *__restrict__ segs, const SegPiece *__restrict__ work, int n_work,
                                                       const uint8_t *const *__restrict__ chunk_text, PassPreset Z) {
    struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gn = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = gt; i < Z.n_arrive; i += gn) Z.arrive[i] = ARRIVE_PENDING;
    for (int64_t i = gt; i < Z.n_flag16; i += gn) reinterpret_cast<uint4 *>(Z.flags)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (gt == 0) {
        *Z.ticket = 0u;
        if (Z.cand_count) *Z.cand_count = 0u;
    }
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const SegPiece P = work[w];
        const SegDev *__restrict__ S = segs + P.seg;
        const int64_t len0 = S->len0;
        const uint8_t *src = chunk_text[S->chunk] + S->seg_lo;
        uint8_t *dst = S->buf + S->glen;
        int64_t q_lo, q_hi;
        piece_range(P, len0, q_lo, q_hi);
        for (int64_t q0 = q_lo + (int64_t)threadIdx.x * 16; q0 < q_hi; q0 += (int64_t)blockDim.x * 16) {
            if (q0 + 16 <= len0) *reinterpret_cast<V16 *>(dst + q0) = *reinterpret_cast<const V16 *>(src + q0);
            else for (int64_t q = q0; q < len0; ++q) dst[q] = src[q];
        }
    }
}

// After a pass's walks, one launch (seg_finish_kernel): blocks 0 .. n_work - 1 stitch, the blocks behind them gather.
//
// Stitch: write each segment's owned part of the polished text into the chunk's new text.  With cls_out it also carries the
// position classes over: a new position is traced back through the segment's edits (newest first); if it lands in or
// next to replaced text its 64-position tile is flagged for the rescan, otherwise its old class is copied.  (Flags are only ever
// SET here -- a tile may belong to two segments; seg_init_kernel cleared them.)
//
// Gather: pack the fix records (and aux bytes) of all segments of a pass into compact arrays, turning segment-local
// coordinates into chunk coordinates: index += idx_base, seqno += seq_base, aux_off += aux_base.  One wave per segment.  With `sum`
// (the device's bookkeeping) rec_off / aux_off count from the chunk's first record and the records of the chunks before it are
// added here; without (the host's) they are offsets into the pass's arrays already.
constexpr uint32_t STITCH_MAX_EDITS = 32;   // beyond this the whole segment is flagged (always safe: flagged = recomputed)
__global__ __launch_bounds__(256) void seg_finish_kernel(const SegDev *__restrict__ segs, int n_segs, const SegPiece *__restrict__ work, int n_work,
                                                         uint8_t *const *__restrict__ chunk_out, uint8_t *const *__restrict__ cls_out,
                                                         uint8_t *const *__restrict__ flags, const int64_t *__restrict__ idx_base,
                                                         const uint32_t *__restrict__ seq_base, const uint32_t *__restrict__ rec_off,
                                                         const uint32_t *__restrict__ aux_off, const ChunkSummary *__restrict__ sum, FixRec *out_recs,
                                                         uint8_t *out_aux) {
    struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
    __shared__ EditRec s_edits[STITCH_MAX_EDITS];
    if ((int)blockIdx.x >= n_work) {
        const int lane = threadIdx.x & 63;
        const int s = ((int)blockIdx.x - n_work) * 4 + (threadIdx.x >> 6);
        if (s >= n_segs) return;
        const SegDev *__restrict__ S = segs + s;
        const uint32_t nrec = S->nrec, naux = S->naux;
        if (!(nrec | naux)) return;
        uint32_t rb = rec_off[s], ab = aux_off[s];
        if (sum) {
            const int c = (int)S->chunk;
            uint32_t r = 0, a = 0;
            for (int q = lane; q < c; q += 64) { r += sum[q].nrec; a += sum[q].naux; }
            for (int o = 32; o > 0; o >>= 1) { r += __shfl_xor(r, o); a += __shfl_xor(a, o); }
            rb += r; ab += a;
        }
        const FixRec *recs = S->recs;
        const uint8_t *aux = S->aux;
        const int64_t ib = idx_base[s];
        const uint32_t sb = seq_base[s];
        for (uint32_t r = lane; r < nrec; r += 64) {
            FixRec f = recs[r];
            f.index += ib;
            f.seqno += sb;
            if (f.kind == 'x') f.aux_off += ab;
            out_recs[rb + r] = f;
        }
        for (uint32_t q = lane; q < naux; q += 64) out_aux[ab + q] = aux[q];
        return;
    }
    const SegPiece P = work[blockIdx.x];
    const SegDev *__restrict__ S = segs + P.seg;
    const uint32_t chunk = S->chunk, nedit = S->nedit;
    const int64_t own_lo = S->own_lo, out_off = S->out_off, gs = S->gs, glen = S->glen, seg_lo = S->seg_lo, cls_n = S->cls_n;
    const int64_t n = S->own_hi - own_lo;
    const uint8_t *buf = S->buf, *cls = S->cls;
    uint8_t *dst = chunk_out[chunk] + out_off;
    uint8_t *cdst = cls_out ? cls_out[chunk] + out_off : nullptr;
    uint8_t *fl = cls_out ? flags[chunk] : nullptr;
    const bool all_dirty = nedit > STITCH_MAX_EDITS;
    const int ne = (cdst && !all_dirty) ? (int)nedit : 0;
    if ((int)threadIdx.x < ne) s_edits[threadIdx.x] = S->edits[threadIdx.x];
    __syncthreads();
    int64_t q_lo, q_hi;
    piece_range(P, n, q_lo, q_hi);
    for (int64_t q0 = q_lo + (int64_t)threadIdx.x * 16; q0 < q_hi; q0 += (int64_t)blockDim.x * 16) {
        const int64_t p0 = own_lo + q0;
        const bool full = q0 + 16 <= n;
        bool text_done = false, cls_done = !cdst;
        if (full && (p0 + 16 <= gs || p0 >= gs)) {                 // sixteen text bytes on one side of the gap
            *reinterpret_cast<V16 *>(dst + q0) = *reinterpret_cast<const V16 *>(buf + (p0 < gs ? p0 : p0 + glen));
            text_done = true;
        }
        if (full && cdst && !all_dirty) {
            // sixteen classes with one common shift: trace the block's two ends through the edits together; as long as
            // both lie on the same side of every edit (and outside its one-position margin) so does everything between
            int64_t lA = p0, lB = p0 + 15;
            bool uniform = true;
            for (int e = ne - 1; e >= 0; --e) {
                const EditRec E = s_edits[e];
                if (lA > E.a + E.plen) { const int64_t d = (int64_t)E.plen - E.oldlen; lA -= d; lB -= d; }
                else if (lB < E.a - 1) { }
                else { uniform = false; break; }
            }
            if (uniform && seg_lo + lB < cls_n) {
                *reinterpret_cast<V16 *>(cdst + q0) = *reinterpret_cast<const V16 *>(cls + seg_lo + lA);
                cls_done = true;
            }
        }
        if (text_done && cls_done) continue;
        const int64_t qe = q0 + 16 < n ? q0 + 16 : n;
        for (int64_t q = q0; q < qe; ++q) {
            const int64_t p = own_lo + q;
            if (!text_done) dst[q] = buf[p < gs ? p : p + glen];
            if (cls_done) continue;
            int64_t l = p;
            bool dirty = all_dirty;
            if (!dirty)
                for (int e = ne - 1; e >= 0; --e) {
                    const EditRec E = s_edits[e];
                    if (l > E.a + E.plen) l -= (int64_t)E.plen - E.oldlen;
                    else if (l >= E.a - 1) { dirty = true; break; }
                }
            if (dirty) {
                fl[(out_off + q) >> 6] = 1;
                cdst[q] = PC_OTHER;
            } else {
                const int64_t old = seg_lo + l;
                cdst[q] = old < cls_n ? cls[old] : (uint8_t)PC_OTHER;
            }
        }
    }
}

// ---- after the walks: what the host's bookkeeping loop did, on the device -----------------------------------------------
// One wave per chunk record, 64 of its segments at a time (running sums by wave prefix scans); then lane 0 of block 0's last
// arriver would have to scan the chunks -- instead rec_off / aux_off stay relative to the chunk's first record, and the one consumer
// (the gather of seg_finish_kernel) adds up the ChunkSummary totals of the chunks BEFORE its own (n_chunks is small: the chunk
// records of one polish call).
__device__ __forceinline__ long long wave_scan_incl64(long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(v, o); if (lane >= o) v += u; }
    return v;
}
__global__ __launch_bounds__(64) void seg_summary_kernel(SegDev *segs, const int32_t *first_seg, int n_chunks, int64_t *idx_base, uint32_t *seq_base,
                                                         uint32_t *rec_off, uint32_t *aux_off, ChunkSummary *out) {
    const int c = blockIdx.x;
    if (c >= n_chunks) return;
    const int lane = threadIdx.x;
    const int s0 = first_seg[c], s1 = first_seg[c + 1];
    long long newlen = 0, shift = 0, seqc = 0, recc = 0, auxc = 0, wrong = 0, lookups = 0;
    int bad = -1, spec = 0;
    for (int base = s0; base < s1; base += 64) {
        const int s = base + lane;
        const bool in = s < s1;
        long long d = 0, own = 0, nrec = 0, naux = 0, seg_lo = 0, own_hi = 0;
        if (in) {
            SegDev &S = segs[s];
            d = S.len - S.len0;
            own_hi = S.last ? S.len : S.own_hi0 + d;
            own = own_hi - S.own_lo;
            nrec = S.nrec; naux = S.naux; seg_lo = S.seg_lo;
            wrong += S.wrong; lookups += (long long)S.lookups;
            if (S.status != PS_OK && (bad < 0 || s < bad)) bad = s;
            if (S.spec_fail && S.status == PS_OK) spec = 1;
        }
        const long long i_own = wave_scan_incl64(own), i_d = wave_scan_incl64(d), i_rec = wave_scan_incl64(nrec), i_aux = wave_scan_incl64(naux);
        if (in) {
            SegDev &S = segs[s];
            S.own_hi = own_hi;
            S.out_off = newlen + i_own - own;
            idx_base[s] = seg_lo + shift + i_d - d;
            seq_base[s] = (uint32_t)(seqc + i_rec - nrec);
            rec_off[s] = (uint32_t)(recc + i_rec - nrec);          // (relative to the chunk: the gather adds the chunks before it)
            aux_off[s] = (uint32_t)(auxc + i_aux - naux);
        }
        newlen += __shfl(i_own, 63); shift += __shfl(i_d, 63);
        seqc += __shfl(i_rec, 63); recc += __shfl(i_rec, 63); auxc += __shfl(i_aux, 63);
    }
    for (int o = 32; o > 0; o >>= 1) {
        wrong += __shfl_xor(wrong, o); lookups += __shfl_xor(lookups, o);
        const int b2 = __shfl_xor(bad, o);
        bad = bad < 0 ? b2 : (b2 < 0 ? bad : (b2 < bad ? b2 : bad));
        spec |= __shfl_xor(spec, o);
    }
    if (lane == 0) {
        ChunkSummary R;
        R.newlen = newlen; R.wrong = wrong; R.lookups = (uint64_t)lookups; R.nrec = (uint32_t)recc; R.naux = (uint32_t)auxc; R.bad_seg = bad; R.spec_fail = spec;
        out[c] = R;
    }
}
// ---- batched variants: blockIdx.y walks the chunks of the batch ---------------------------------------------------
// Pass 0: count AND class of every window in one kernel.  A block takes the windows that END at origin .. origin + 4095, origin =
// tile * SC_STRIDE - 64: thread t rolls through its 16 of them as before (hash four, four home-slot loads in flight, resolve), the
// counts go to LDS, and after a barrier every window is classed from its own count and the count of the window k back (k <= 64:
// inside the block's 64 halo windows, which the block before it classes).  The counts never leave the CU: 1 byte per window is
// written instead of 5, and the separate pass over them (classify: 0.17 ms for 47 Mb) is gone.
constexpr int SC_BACK = 64;                          // halo windows of a block (>= the largest k)
constexpr int SC_STRIDE = SC_TILE - SC_BACK;         // new windows per block
__global__ __launch_bounds__(SC_THREADS) void scan_classify_batch_kernel(const ScanChunk *__restrict__ chunks, int n_chunks, TableDev T, uint32_t solid) {
    __shared__ uint32_t s_code[SC_THREADS + SC_HALO];
    __shared__ uint32_t s_inv[SC_THREADS + SC_HALO];
    __shared__ uint32_t s_cnt[SC_TILE];              // count of the window that ends at origin + i
    __shared__ uint8_t s_ok[SC_TILE];                // ... and whether there is a window, and a k-mer in it
    const int t = threadIdx.x;
    const int k = T.k;
    const u128 kmask = maskbits(2 * k);
    for (int ci = blockIdx.y; ci < n_chunks; ci += gridDim.y) {
        const ScanChunk C = chunks[ci];
        const uint8_t *__restrict__ text = C.text;
        const int64_t n = C.len;
        const int64_t nwin = n - k + 1;
        if (nwin <= 0) continue;
        const int64_t ntiles = (n + SC_STRIDE - 1) / SC_STRIDE;
        for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            const int64_t origin = tile * SC_STRIDE - SC_BACK;
            uint32_t c, iv;
            stage16(text, origin + (int64_t)t * SC_GROUP, n, c, iv);
            s_code[t + SC_HALO] = c;
            s_inv[t + SC_HALO] = iv;
            if (t < SC_HALO) {
                uint32_t hc, hiv;
                stage16(text, origin - (int64_t)(SC_HALO - t) * SC_GROUP, n, hc, hiv);
                s_code[t] = hc;
                s_inv[t] = hiv;
            }
            __syncthreads();
            const uint32_t w4 = s_code[t], w3 = s_code[t + 1], w2 = s_code[t + 2], w1 = s_code[t + 3];
            const uint64_t ivprev = ((uint64_t)s_inv[t] << 48) | ((uint64_t)s_inv[t + 1] << 32) | ((uint64_t)s_inv[t + 2] << 16) |
                                    (uint64_t)s_inv[t + 3];
            u128 fwd = band(mk(((uint64_t)w4 << 32) | w3, ((uint64_t)w2 << 32) | w1), kmask);
            u128 rc = revcomp(fwd, k);
            int run = ivprev ? (int)__builtin_ctzll(ivprev) : 64;
            const int64_t e0 = origin + (int64_t)t * SC_GROUP;
#pragma unroll
            for (int j0 = 0; j0 < SC_GROUP; j0 += 4) {
                u128 hs[4];
                bool ok[4];
                ulonglong2 ent[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u;
                    const uint32_t cj = (c >> (30 - 2 * j)) & 3u;
                    const bool bad = (iv >> (15 - j)) & 1u;
                    fwd = band(bor(shl(fwd, 2), mk(0, cj)), kmask);
                    rc = bor(shr(rc, 2), shl(mk(0, 3u - cj), 2 * (k - 1)));
                    run = bad ? 0 : run + 1;
                    const int64_t e = e0 + j;
                    ok[u] = run >= k && e - k + 1 >= 0 && e < n;
                    hs[u] = mix(lt(rc, fwd) ? rc : fwd, T.B);
                    ent[u] = make_ulonglong2(0ull, 0ull);
                    if (ok[u]) ent[u] = *reinterpret_cast<const ulonglong2 *>(read_slots(T, hs[u]) + 2 * home_of(hs[u], T.B, T.s));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s_cnt[t * SC_GROUP + j0 + u] = ok[u] ? clamp32(table_get_prefetched(T, hs[u], ent[u])) : 0u;
                    s_ok[t * SC_GROUP + j0 + u] = ok[u] ? 1 : 0;
                }
            }
            __syncthreads();
            // classes of my 16 windows (the halo's were written by the block before this one)
            if (t >= SC_BACK / SC_GROUP) {
                struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
                V16 out;
                out.w[0] = out.w[1] = out.w[2] = out.w[3] = 0;
                const int64_t p0 = e0 - k + 1;                               // position of my first window
#pragma unroll
                for (int j = 0; j < SC_GROUP; ++j) {
                    const int64_t p = p0 + j;
                    const uint32_t me = s_cnt[t * SC_GROUP + j];
                    uint8_t cl;
                    if (!s_ok[t * SC_GROUP + j]) cl = PC_OTHER;
                    else if (me < solid) cl = PC_BAD;
                    else if (p > 0) {
                        // the window k back, or window 0 (src/jasper.py:80: seq[max(0, i-k):max(k, i)])
                        const int64_t qe = (p - k > 0 ? p - k : 0) + k - 1;   // where that window ends
                        const int qi = (int)(qe - origin);
                        cl = (!s_ok[qi] || 50ull * me < (unsigned long long)s_cnt[qi]) ? PC_OTHER : PC_CLEAN;
                    } else cl = PC_CLEAN;
                    out.w[j >> 2] |= (uint32_t)cl << (8 * (j & 3));
                }
                if (p0 >= 0 && p0 + SC_GROUP <= nwin) *reinterpret_cast<V16 *>(C.cls + p0) = out;
                else {
#pragma unroll
                    for (int j = 0; j < SC_GROUP; ++j) {
                        const int64_t p = p0 + j;
                        if (p >= 0 && p < nwin) C.cls[p] = (uint8_t)((out.w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// (bx of gx: the block's place among the blocks of find_cuts_batch_kernel that look for sync points)
__device__ __forceinline__ void find_sync_blocks(const ScanChunk *__restrict__ chunks, int n_chunks, int k, int bx, int gx) {
    struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
    const int64_t W = 4ll * k;
    for (int ci = blockIdx.y; ci < n_chunks; ci += gridDim.y) {
        const ScanChunk C = chunks[ci];
        if (!C.want_sync) continue;
        const int64_t nwin = C.len - k + 1;
        const uint8_t *__restrict__ cls = C.cls;
        static_assert(PC_CLEAN == 0 && PC_BAD == 1 && PC_OTHER == 2, "the block test below looks at bit 0 of the class bytes");
        // sixteen positions per thread: a candidate is a BAD position whose left neighbour is CLEAN -- rare, so most
        // blocks are rejected after one 16-B load
        const int64_t nblk = (nwin + 15) >> 4;
        for (int64_t blk = bx * (int64_t)blockDim.x + threadIdx.x; blk < nblk; blk += (int64_t)gx * blockDim.x) {
            const int64_t p0 = blk << 4;
            uint32_t w[4];
            if (p0 + 16 <= nwin) {
                const V16 v = *reinterpret_cast<const V16 *>(cls + p0);
                w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3];
                if (!((w[0] | w[1] | w[2] | w[3]) & 0x01010101u)) continue;       // no BAD (= 1; CLEAN 0, OTHER 2) in the block
            }
            const int64_t pe = p0 + 16 < nwin ? p0 + 16 : nwin;
            for (int64_t p = p0; p < pe; ++p) {
                if (p < W || p + k - 1 > nwin) continue;
                if (cls[p] != PC_BAD || cls[p - 1] != PC_CLEAN) continue;
                // cls[p+1 .. p+k-2] all BAD and cls[p-W .. p-2] all CLEAN: sixteen bytes per load, all loads independent (byte after
                // byte with an early exit this was a chain of up to 4k + k load latencies per candidate)
                uint32_t diff = 0;
                {
                    int64_t q = p + 1;
                    const int64_t qe = p + k - 1;
                    for (; q + 16 <= qe; q += 16) {
                        const V16 v = *reinterpret_cast<const V16 *>(cls + q);
                        diff |= (v.w[0] ^ 0x01010101u) | (v.w[1] ^ 0x01010101u) | (v.w[2] ^ 0x01010101u) | (v.w[3] ^ 0x01010101u);
                    }
                    for (; q < qe; ++q) diff |= (uint32_t)(cls[q] ^ (uint8_t)PC_BAD);
                    q = p - W;
                    const int64_t qf = p - 1;
                    for (; q + 16 <= qf; q += 16) {
                        const V16 v = *reinterpret_cast<const V16 *>(cls + q);
                        diff |= v.w[0] | v.w[1] | v.w[2] | v.w[3];
                    }
                    for (; q < qf; ++q) diff |= (uint32_t)cls[q];
                }
                if (diff) continue;
                const unsigned int idx = atomicAdd(C.cand_count, 1u);        // ONE list for the whole batch: (chunk << 40) | position
                if (idx < C.cand_cap) C.cand[idx] = ((int64_t)ci << 40) | p;
            }
        }
    }
}

// Classes next to changed text: one wave per 64-window tile; a tile is recomputed when it or a neighbouring tile holds
// changed text (k <= 64, so a changed base at P affects the windows P-k+1..P and, through the count k back, up to P+k).
__global__ __launch_bounds__(256) void rescan_batch_kernel(const ScanChunk *__restrict__ chunks, int n_chunks, TableDev T, uint32_t solid) {
    __shared__ uint32_t s_cnt[4][128];
    __shared__ uint8_t s_valid[4][128];
    __shared__ uint8_t s_text[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = T.k;
    for (int ci = blockIdx.y; ci < n_chunks; ci += gridDim.y) {
        const ScanChunk C = chunks[ci];
        const int64_t nwin = C.len - k + 1;
        if (nwin <= 0) continue;
        const int64_t ntile = (nwin + 63) >> 6, nflag = (C.len >> 6) + 1;
        // (a wave looks at the flags of 64 tiles at once -- one per lane -- and then takes the flagged ones in turn: tile after tile
        //  through one wave is a chain of flag-load latencies)
        // (the 64 are a wave's next tiles of the round-robin over all waves, W apart: changed text comes in clusters -- a segment
        //  flagged whole is 200 adjacent tiles -- and neighbours must not end up in one wave)
        const int64_t W = (int64_t)gridDim.x * 4;
        for (int64_t tile0 = (int64_t)blockIdx.x * 4 + wave; tile0 < ntile; tile0 += 64 * W) {
            uint8_t f = 0;
            {
                const int64_t tl = tile0 + (int64_t)lane * W;
                if (tl < ntile) {
                    f = C.flags[tl];
                    if (tl > 0) f |= C.flags[tl - 1];
                    if (tl + 1 < nflag) f |= C.flags[tl + 1];
                }
            }
            unsigned long long todo = __ballot(f != 0);
          while (todo) {
            const int64_t tile = tile0 + (int64_t)__builtin_ctzll(todo) * W;
            todo &= todo - 1ull;
            const int64_t base = tile * 64 - 64;
            // the text under the tile's 128 windows (128 + k - 1 <= 191 bytes) comes into LDS with one round of loads: a lane that
            // read its window's k bytes itself, one after the other, spent ~100 us per tile waiting for them
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t pos = base + (int64_t)lane * 4 + q;
                s_text[wave][lane * 4 + q] = (pos >= 0 && pos < C.len) ? C.text[pos] : (uint8_t)'N';
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int64_t p = base + r * 64 + lane;
                uint32_t cnt = 0;
                uint8_t valid = 0;
                if (p >= 0 && p < nwin) {
                    u128 fwd = mk(0, 0);
                    bool ok = true;
                    for (int j = 0; j < k; ++j) {
                        const int c = code(s_text[wave][r * 64 + lane + j]);
                        ok = ok && c >= 0;
                        fwd = bor(shl(fwd, 2), mk(0, (uint64_t)(c & 3)));
                    }
                    if (ok) {
                        cnt = clamp32(table_get(T, mix(canonical(fwd, k), T.B)));
                        valid = 1;
                    }
                }
                s_cnt[wave][r * 64 + lane] = cnt;
                s_valid[wave][r * 64 + lane] = valid;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const int64_t p = tile * 64 + lane;
            if (p < nwin) {
                const int me = 64 + lane;
                uint8_t c;
                if (!s_valid[wave][me]) c = PC_OTHER;
                else if (s_cnt[wave][me] < solid) c = PC_BAD;
                else if (p > 0) {
                    const int qi = p - k > 0 ? me - k : 64;       // window k back, or window 0 (only reachable in tile 0)
                    c = (!s_valid[wave][qi] || 50ull * s_cnt[wave][me] < (unsigned long long)s_cnt[wave][qi]) ? PC_OTHER : PC_CLEAN;
                } else c = PC_CLEAN;
                C.cls[p] = c;
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
    }
}

// clean-zone boundaries: per CLEAN_CELL positions of a chunk, a position p (searched from the middle of the cell) whose
// window starts [p-4k, p+k) are all CLEAN.  No event can happen there whatever stride phase the walk arrives with, so
// a chunk may be cut at p if the segment to the right takes its start position from the one to the left (SegDev::chain_in).
// (one wave per cell: wx of gw = the wave's place among the waves of find_cuts_batch_kernel that look for clean zones)
__device__ __forceinline__ void find_clean_waves(const ScanChunk *__restrict__ chunks, int n_chunks, int k, int wx, int gw) {
    const int lane = threadIdx.x & 63;
    for (int ci = blockIdx.y; ci < n_chunks; ci += gridDim.y) {
        const ScanChunk C = chunks[ci];
        const int64_t nwin = C.len - k + 1;
        for (uint32_t g = (uint32_t)wx; g < C.n_cells; g += (uint32_t)gw) {
            int64_t p0 = (int64_t)g * CLEAN_CELL + CLEAN_CELL / 2;
            const int64_t cell_end = (int64_t)(g + 1) * CLEAN_CELL;
            int64_t cand = -1;
            for (int attempt = 0; attempt < 8; ++attempt) {
                if (p0 - 4ll * k < 0 || p0 + k > nwin || p0 + k > cell_end) break;
                int64_t last_bad = -1;
                for (int64_t q0 = p0 - 4ll * k; q0 < p0 + k; q0 += 64) {
                    const int64_t q = q0 + lane;
                    const bool nc = q < p0 + k && C.cls[q] != PC_CLEAN;
                    const uint64_t m = __ballot(nc);
                    if (m) last_bad = q0 + 63 - (int64_t)__builtin_clzll(m);
                }
                if (last_bad < 0) { cand = p0; break; }
                p0 = last_bad + 4ll * k + 1;
            }
            if (lane == 0) C.clean_cand[g] = cand;
        }
    }
}

// Both searches read the classes the scan in front of them wrote and nothing of each other: one launch, the first sync_gx blocks
// of a row look for sync points, the rest -- four waves each -- for clean zones.  (Not inside the scan: a candidate's 4k
// neighbourhood crosses its blocks.)
__global__ __launch_bounds__(256) void find_cuts_batch_kernel(const ScanChunk *__restrict__ chunks, int n_chunks, int k, int sync_gx) {
    if ((int)blockIdx.x < sync_gx) find_sync_blocks(chunks, n_chunks, k, (int)blockIdx.x, sync_gx);
    else find_clean_waves(chunks, n_chunks, k, ((int)blockIdx.x - sync_gx) * 4 + (int)(threadIdx.x >> 6), ((int)gridDim.x - sync_gx) * 4);
}

static void launch_find_cuts(const ScanChunk *d_chunks, int n_chunks, int k, int gx, int gy, hipStream_t stream) {
    const int clean_gx = (std::max(1, 8192 / gy) + 3) / 4;
    hipLaunchKernelGGL(find_cuts_batch_kernel, dim3(gx + clean_gx, gy), dim3(256), 0, stream, d_chunks, n_chunks, k, gx);
}

void launch_rescan_batch(const TableDev &T, const ScanChunk *d_chunks, int n_chunks, int k, uint32_t solid, hipStream_t stream) {
    if (n_chunks <= 0) return;
    const int gy = n_chunks < 1024 ? n_chunks : 1024;
    const int gx = std::max(1, 4096 / gy);
    hipLaunchKernelGGL(rescan_batch_kernel, dim3(gx, gy), dim3(256), 0, stream, d_chunks, n_chunks, T, solid);
    launch_find_cuts(d_chunks, n_chunks, k, gx, gy, stream);
}

void launch_scan_batch(const TableDev &T, const ScanChunk *d_chunks, int n_chunks, int k, uint32_t solid, hipStream_t stream) {
    if (n_chunks <= 0) return;
    const int gy = n_chunks < 1024 ? n_chunks : 1024;
    const int gx = std::max(1, 4096 / gy);
    hipLaunchKernelGGL(scan_classify_batch_kernel, dim3(gx, gy), dim3(SC_THREADS), 0, stream, d_chunks, n_chunks, T, solid);
    launch_find_cuts(d_chunks, n_chunks, k, gx, gy, stream);
}

// chunk texts <-> one packed buffer (text of chunk c at pack + offs[c]): a batch of very many small records crosses PCIe in one
// transfer instead of one per record (polish_host.hip)
__global__ __launch_bounds__(256) void copy_chunks_kernel(uint8_t *const *__restrict__ chunk_ptr, uint8_t *__restrict__ pack, const int64_t *__restrict__ offs, int n,
                                                          int to_chunks) {
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const int64_t len = offs[c + 1] - offs[c];
        uint8_t *a = chunk_ptr[c], *b = pack + offs[c];
        const uint8_t *src = to_chunks ? b : a;
        uint8_t *dst = to_chunks ? a : b;
        for (int64_t i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
    }
}
void launch_copy_chunks(uint8_t *const *d_chunk_ptr, uint8_t *d_pack, const int64_t *d_offs, int n, bool to_chunks, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(copy_chunks_kernel, dim3((unsigned)std::min(n, 256 * 16)), dim3(256), 0, stream, d_chunk_ptr, d_pack, d_offs, n, to_chunks ? 1 : 0);
}

void launch_seg_init(const SegDev *d_segs, const SegPiece *d_work, int n_work, const uint8_t *const *d_chunk_text, const PassPreset &preset,
                     hipStream_t stream) {
    if (n_work <= 0) return;
    hipLaunchKernelGGL(seg_init_kernel, dim3(n_work), dim3(256), 0, stream, d_segs, d_work, n_work, d_chunk_text, preset);
}
void launch_seg_walk(const TableDev &T, SegDev *d_segs, int n_segs, PolishParams pp, int pass, ScratchPool pool, unsigned int *d_ticket,
                     hipStream_t stream) {
    if (n_segs <= 0) return;
    hipLaunchKernelGGL(seg_walk_kernel, dim3(n_segs), dim3(64), 0, stream, T, d_segs, n_segs, pp, pass, pool, d_ticket);
}
void launch_seg_summary(SegDev *d_segs, int n_segs, const int32_t *d_first_seg, int n_chunks, int64_t *idx_base, uint32_t *seq_base, uint32_t *rec_off,
                        uint32_t *aux_off, ChunkSummary *d_out, hipStream_t stream) {
    if (n_segs <= 0 || n_chunks <= 0) return;
    hipLaunchKernelGGL(seg_summary_kernel, dim3(n_chunks), dim3(64), 0, stream, d_segs, d_first_seg, n_chunks, idx_base, seq_base, rec_off, aux_off, d_out);
}
void launch_seg_finish(const SegDev *d_segs, int n_segs, const SegPiece *d_work, int n_work, uint8_t *const *d_chunk_out, uint8_t *const *d_cls_out,
                       uint8_t *const *d_flags, const int64_t *idx_base, const uint32_t *seq_base, const uint32_t *rec_off, const uint32_t *aux_off,
                       const ChunkSummary *d_sum, FixRec *out_recs, uint8_t *out_aux, hipStream_t stream) {
    if (n_segs <= 0 || n_work <= 0) return;
    const int gather_blocks = out_recs ? (n_segs + 3) / 4 : 0;
    hipLaunchKernelGGL(seg_finish_kernel, dim3(n_work + gather_blocks), dim3(256), 0, stream, d_segs, n_segs, d_work, n_work, d_chunk_out, d_cls_out, d_flags,
                       idx_base, seq_base, rec_off, aux_off, d_sum, out_recs, out_aux);
}

}  // namespace jk
