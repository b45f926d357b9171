// repair.hip -- the repair stage: the scans' error records applied to the text in HBM, in rounds (semantics: include/jasper_hip.h,
// jasper_repair).
//
// An extension.  The reference repairs inside its walk and never looks at the text again; the scans of this library list what the walk has
// left.  A round here is: indel_scan_device with its mixed half (it carries the variant scan) and compound_scan_device (it carries the
// dense report) on the current text; the records of kind error made edits and chosen on the host (repair_host.hpp); and
//
//   repair_apply_kernel     one workgroup per tile of REPAIR_TILE OUTPUT bytes, lane l the 16 bytes from tile + 16 l on, written as one
//                           aligned 16-byte store.  The host has planned, per edit, where its y starts in the new text (dst) and what has
//                           to be added to an output position behind y to get the input position it is copied from (delta); the list is
//                           in dst order with an entry {0, 0, no y} before it and one that no position reaches behind it, so every output
//                           byte has a governing entry: the last one with dst <= the byte.  A tile finds its first and last governing
//                           entry by binary search (its first wave, 64 pivots a step) and goes through them in chunks of REPAIR_CHUNK staged into LDS -- a loop, because a
//                           tile of 1-byte gaps between 64-byte deletions is governed by about as many entries as it has bytes.  In a
//                           chunk a lane looks its first byte up in the staged dst (binary search) and then either has all 16 bytes
//                           behind one y and before the next entry -- one 16-byte load at a shifted, generally misaligned address, the
//                           case of nearly every lane of a real text -- or goes byte by byte, moving to the next entry as it passes its
//                           dst: a base of y (2 bits -> letter) or an input byte, taken from 16 bytes that are loaded
//                           once per stretch the lane copies.
//
// Per round only records come down and edits go up; the text stays in two workspace buffers that take turns.  Bytes that are not replaced are
// copied as they stand.
#include "repair.hpp"
#include "scan_tile.hpp"

namespace jk {

struct EditDev {
    int64_t dst;                   // first output byte of y
    int64_t delta;                 // output position p >= dst + ylen (and before the next entry's dst) is input byte p + delta
    uint64_t bases[2];
    uint32_t ylen, pad;
};
static_assert(sizeof(EditDev) == 40, "uploaded as it is");

// The last entry of ed[lo .. n) with dst <= p, given ed[lo].dst <= p, by one whole wave: a binary search with 64 pivots a step -- lane l
// probes the (l + 1)-th of 64 evenly spaced entries, the ballot is a prefix of ones because dst ascends, and its popcount picks the
// sixty-fourth of the range to go on with.  Three dependent loads for 100 000 entries instead of seventeen: a tile's two searches are
// latency, and every tile waits for them before it moves a byte.
__device__ __forceinline__ int64_t governing(const EditDev *__restrict__ ed, int64_t lo, int64_t n, int64_t p, int lane) {
    int64_t hi = n;                                     // ed[lo].dst <= p < ed[hi].dst (hi == n: no such entry)
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t at = lo + (int64_t)(lane + 1) * step;
        const int c = __popcll(__ballot(at < hi && ed[at].dst <= p));
        const int64_t up = lo + (int64_t)(c + 1) * step;
        lo += (int64_t)c * step;
        hi = up < hi ? up : hi;
    }
    return lo;
}

__global__ __launch_bounds__(REPAIR_THREADS) void repair_apply_kernel(const uint8_t *__restrict__ in, int64_t n_in, uint8_t *__restrict__ out, int64_t n_out,
                                                                      const EditDev *__restrict__ ed, int64_t n_ed) {
    __shared__ int64_t s_dst[REPAIR_CHUNK + 1], s_delta[REPAIR_CHUNK];
    __shared__ uint64_t s_b0[REPAIR_CHUNK], s_b1[REPAIR_CHUNK];
    __shared__ uint32_t s_ylen[REPAIR_CHUNK];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * REPAIR_TILE;
    if (t0 >= n_out) return;                            // (block-uniform)
    const int64_t t1 = t0 + REPAIR_TILE < n_out ? t0 + REPAIR_TILE : n_out;
    __shared__ int64_t s_gov[2];
    if (tid < 64) {                                     // (the first wave, whole)
        const int64_t first = governing(ed, 0, n_ed - 1, t0, tid);      // (the entry behind the list governs nothing)
        const int64_t near = first + 64 < n_ed - 1 ? first + 64 : n_ed - 1;      // the last one is nearly always among the next 64: one step
        const int64_t last = near == n_ed - 1 || ed[near].dst > t1 - 1 ? governing(ed, first, near, t1 - 1, tid) : governing(ed, near, n_ed - 1, t1 - 1, tid);
        if (tid == 0) {
            s_gov[0] = first;
            s_gov[1] = last;
        }
    }
    __syncthreads();
    const int64_t lo = s_gov[0], hi = s_gov[1];
    const int64_t o = t0 + 16 * (int64_t)tid;
    const int64_t oe = o + 16 < n_out ? o + 16 : n_out;                                        // this lane's bytes: [o, oe)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int64_t c0 = lo; c0 <= hi; c0 += REPAIR_CHUNK) {
        const int cn = (int)(hi + 1 - c0 < REPAIR_CHUNK ? hi + 1 - c0 : REPAIR_CHUNK);
        __syncthreads();                                // the chunk before has been read
        if (tid < cn) {
            const EditDev e = ed[c0 + tid];
            s_dst[tid] = e.dst;
            s_delta[tid] = e.delta;
            s_b0[tid] = e.bases[0];
            s_b1[tid] = e.bases[1];
            s_ylen[tid] = e.ylen;
        }
        if (tid == 0) s_dst[cn] = ed[c0 + cn].dst;      // (c0 + cn <= hi + 1 <= n_ed - 1: the entry behind the list at the latest)
        __syncthreads();
        const int64_t a = o > s_dst[0] ? o : s_dst[0];  // the bytes of this lane that this chunk governs: [a, b)
        const int64_t b = oe < s_dst[cn] ? oe : s_dst[cn];
        if (a >= b) continue;
        int i = 0, j = cn;                              // s_dst[i] <= a < s_dst[j]
        while (j - i > 1) {
            const int mid = (i + j) >> 1;
            if (s_dst[mid] <= a) i = mid;
            else j = mid;
        }
        const int64_t from = a + s_delta[i];
        if (b - a == 16 && a >= s_dst[i] + (int64_t)s_ylen[i] && s_dst[i + 1] >= b && from >= 0 && from + 16 <= n_in) {
            struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
            const V16 v = *reinterpret_cast<const V16 *>(in + from);
            w[0] = v.w[0]; w[1] = v.w[1]; w[2] = v.w[2]; w[3] = v.w[3];
            continue;
        }
        Raw16 v;                                        // the 16 input bytes from vb on, loaded when a byte outside them is asked for
        int64_t vb = -16;
        for (int64_t p = a; p < b; ++p) {
            while (i + 1 < cn && s_dst[i + 1] <= p) ++i;
            const int64_t iny = p - s_dst[i];
            uint32_t ch;
            if (iny < (int64_t)s_ylen[i]) {
                const uint64_t bits = iny < 32 ? s_b0[i] : s_b1[i];
                ch = (0x54474341u >> (8 * (uint32_t)((bits >> (2 * (iny & 31))) & 3ull))) & 0xFFu;      // "ACGT"
            } else {
                const int64_t q = p + s_delta[i];       // (the host's plan maps every such byte into the input: 0 <= q < n_in)
                if (q < vb || q >= vb + 16) {
                    vb = q;
                    v = load16(in, q, n_in);            // (bounds-checked; a lane loads once per stretch it copies, not once per byte)
                }
                const int at = (int)(q - vb);
                const uint32_t word = at < 8 ? (at < 4 ? v.w[0] : v.w[1]) : (at < 12 ? v.w[2] : v.w[3]);      // (selects: no register array indexed dynamically)
                ch = (word >> (8 * (at & 3))) & 0xFFu;
            }
            const int at = (int)(p - o);
            w[at >> 2] |= ch << (8 * (at & 3));
        }
    }
    if (o < n_out) *reinterpret_cast<uint4 *>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);      // (16 bytes of slack lie behind the text)
}

static uint64_t unreliable_of(const ReportOut &R) {
    uint64_t n = 0;
    for (size_t i = 2; i < R.counts.size(); i += 4) n += R.counts[i];
    return n;
}

// The checked and planned list applied: the n_in bytes from d_in on -> workspace slot out_slot of T (n_out bytes and 16 of slack), on T's
// stream; waits for it.  Adds the kernel's event time to `seconds`.
static int launch_apply(Table &T, int out_slot, const uint8_t *d_in, int64_t n_in, const Edit *edits, uint64_t n, const EditPlan &P, uint8_t *&d_out, double &seconds,
                        std::string &err) {
    const int64_t n_out = P.new_offsets.back();
    d_out = (uint8_t *)T.workspace(out_slot, (size_t)n_out + 16, err);
    if (!d_out) return -1;
    if (n_out == 0) return 0;
    std::vector<EditDev> ed(n + 2);
    ed[0] = EditDev{0, 0, {0, 0}, 0, 0};
    for (uint64_t i = 0; i < n; ++i)
        ed[i + 1] = EditDev{P.dst[i], P.src[i] + (int64_t)edits[i].ref_len - (P.dst[i] + (int64_t)edits[i].len), {edits[i].bases[0], edits[i].bases[1]}, edits[i].len, 0};
    ed[n + 1] = EditDev{INT64_MAX, 0, {0, 0}, 0, 0};
    EditDev *d_ed = (EditDev *)T.workspace(Table::WS_REPAIR + 2, ed.size() * sizeof(EditDev), err);
    if (!d_ed) return -1;
    hipStream_t st = T.stream;
    Events ev;
    if (ev.create(err)) return -1;
    HIPCHK(hipMemcpyAsync(d_ed, ed.data(), ed.size() * sizeof(EditDev), hipMemcpyHostToDevice, st));
    const uint64_t ntiles = ((uint64_t)n_out + REPAIR_TILE - 1) / REPAIR_TILE;
    if (ntiles > 0x7FFFFFFFull) { err = "apply edits: text too long"; return -1; }
    HIPCHK(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(repair_apply_kernel, dim3((unsigned)ntiles), dim3(REPAIR_THREADS), 0, st, d_in, n_in, d_out, n_out, d_ed, (int64_t)ed.size());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], st));
    HIPCHK(jk_stream_wait(st));                         // (`ed` is read until here)
    return ev.add_seconds(seconds, err);
}

static int fetch_text(Table &T, const uint8_t *d_text, const std::vector<int64_t> &offs, RepairOut &out, std::string &err) {
    out.offsets = offs;
    out.text.resize((size_t)offs.back());
    if (!out.text.empty()) HIPCHK(hipMemcpyAsync(&out.text[0], d_text, out.text.size(), hipMemcpyDeviceToHost, T.stream));
    HIPCHK(jk_stream_wait(T.stream));
    return 0;
}

static int offsets_from_zero(int n_seqs, const int64_t *offsets, const char *what, std::vector<int64_t> &offs, std::string &err) {
    offs.assign((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) { err = std::string(what) + ": offsets must not decrease"; return -1; }
        offs[i + 1] = offsets[i + 1] - offsets[0];
    }
    return 0;
}

static int repair_check_args(const Table &T, uint32_t thre, int indel_max_len, int compound_max_len, int rounds, std::string &err) {
    if (thre < 1) { err = "repair: the threshold (thre) must be at least 1"; return -1; }
    if (T.k < 2) { err = "repair: k must be at least 2"; return -1; }
    if (indel_max_len < 1 || indel_max_len > INDEL_MAX_LEN) { err = "repair: indel_max_len must be in 1..16"; return -1; }
    if (compound_max_len < 1 || compound_max_len > COMPOUND_MAX_LEN) { err = "repair: compound_max_len must be in 1..64"; return -1; }
    if (rounds < 1 || rounds > REPAIR_MAX_ROUNDS) { err = "repair: rounds must be in 1..8"; return -1; }
    return 0;
}

// the loop on a text of T's device that starts at its sequence 0 (offs[0] == 0); the first new text goes to workspace slot `slot`, the next
// one to the other text slot, and so on
static int repair_loop(Table &T, int n_seqs, const uint8_t *d_text, std::vector<int64_t> offs, int slot, uint32_t thre, int indel_max_len, int compound_max_len, int rounds,
                       RepairOut &out, std::string &err) {
    const int W = Table::WS_REPAIR;
    const uint8_t *cur = d_text;
    bool settled = false;                               // `after` is the report of a round that accepted nothing
    for (int r = 1; r <= rounds; ++r) {
        IndelOut io;
        CompoundOut co;
        ReportOut rep;
        if (indel_scan_device(T, n_seqs, cur, offs.data(), thre, indel_max_len, true, 0, io, err)) return -1;
        if (compound_scan_device(T, n_seqs, cur, offs.data(), thre, compound_max_len, rep, co, err)) return -1;
        out.seconds += io.seconds + co.seconds;
        const uint64_t unrel = unreliable_of(rep);
        if (r > 1) out.rounds.back().unreliable_after = unrel;
        std::vector<Edit> edits;
        if (edits_from_variants(io.var.recs, edits, err) || edits_from_indels(io.recs, edits, err) || edits_from_mixed(io.mixed_recs, edits, err) ||
            edits_from_compound(co.recs, edits, err))
            return -1;
        Selection S;
        select_edits(edits, T.k, S);
        out.rounds.push_back(RepairRound{S.records, S.accepted.size(), S.conflicts, S.ambiguous, unrel, unrel});
        if (r == 1) out.before = rep;
        if (S.accepted.empty()) {
            out.after = std::move(rep);
            settled = true;
            break;
        }
        if (check_edits(S.accepted.data(), S.accepted.size(), n_seqs, offs.data(), err)) return -1;      // (what a scan has listed passes)
        EditPlan P;
        plan_edits(S.accepted.data(), S.accepted.size(), n_seqs, offs.data(), P);
        uint8_t *d_new = nullptr;
        double secs = 0;
        if (launch_apply(T, slot, cur, offs.back(), S.accepted.data(), S.accepted.size(), P, d_new, secs, err)) return -1;
        out.apply_seconds += secs;
        out.seconds += secs;
        for (Edit &e : S.accepted) {
            e.round = (uint8_t)r;
            out.edits.push_back(e);
        }
        cur = d_new;
        offs = P.new_offsets;
        slot = slot == W ? W + 1 : W;
    }
    if (!settled) {                                     // the last round still applied edits: one more report of what it left
        if (kmer_report_device(T, n_seqs, cur, offs.data(), thre, out.after, err)) return -1;
        out.seconds += out.after.seconds;
        out.rounds.back().unreliable_after = unreliable_of(out.after);
    }
    return fetch_text(T, cur, offs, out, err);
}

int repair_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int indel_max_len, int compound_max_len, int rounds, RepairOut &out,
                  std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "repair: bad arguments"; return -1; }
    if (repair_check_args(T, thre, indel_max_len, compound_max_len, rounds, err)) return -1;
    out = RepairOut();
    std::vector<int64_t> offs;
    if (offsets_from_zero(n_seqs, offsets, "repair", offs, err)) return -1;
    if (offs.back() && !d_text) { err = "repair: null text"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    return repair_loop(T, n_seqs, n_seqs ? d_text + offsets[0] : d_text, offs, Table::WS_REPAIR, thre, indel_max_len, compound_max_len, rounds, out, err);
}

int repair_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int indel_max_len, int compound_max_len, int rounds, RepairOut &out,
                std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "repair: bad arguments"; return -1; }
    if (repair_check_args(T, thre, indel_max_len, compound_max_len, rounds, err)) return -1;
    out = RepairOut();
    HostText H;
    if (pack_host_text(T, Table::WS_REPAIR, n_seqs, seqs, lens, "repair", H, err)) return -1;
    return repair_loop(T, n_seqs, H.d_text, H.offs, Table::WS_REPAIR + 1, thre, indel_max_len, compound_max_len, rounds, out, err);
}

static int apply_checked(Table &T, int n_seqs, const uint8_t *d_text, const std::vector<int64_t> &offs, const Edit *edits, uint64_t n_edits, RepairOut &out,
                         std::string &err) {
    if (n_edits && !edits) { err = "apply edits: bad arguments"; return -1; }
    if (check_edits(edits, n_edits, n_seqs, offs.data(), err)) return -1;
    EditPlan P;
    plan_edits(edits, n_edits, n_seqs, offs.data(), P);
    uint8_t *d_new = nullptr;
    if (launch_apply(T, Table::WS_REPAIR + 1, d_text, offs.back(), edits, n_edits, P, d_new, out.apply_seconds, err)) return -1;
    out.seconds = out.apply_seconds;
    return fetch_text(T, d_new, P.new_offsets, out, err);
}

int apply_edits_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, const Edit *edits, uint64_t n_edits, RepairOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && !offsets)) { err = "apply edits: bad arguments"; return -1; }
    out = RepairOut();
    std::vector<int64_t> offs;
    if (offsets_from_zero(n_seqs, offsets, "apply edits", offs, err)) return -1;
    if (offs.back() && !d_text) { err = "apply edits: null text"; return -1; }
    HIPCHK(hipSetDevice(T.device));
    return apply_checked(T, n_seqs, n_seqs ? d_text + offsets[0] : d_text, offs, edits, n_edits, out, err);
}

int apply_edits_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, const Edit *edits, uint64_t n_edits, RepairOut &out, std::string &err) {
    if (n_seqs < 0 || (n_seqs && (!seqs || !lens))) { err = "apply edits: bad arguments"; return -1; }
    out = RepairOut();
    // the list is checked before anything goes to the device: a refused list launches and copies nothing
    std::vector<int64_t> offs((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        if (lens[i] < 0 || (lens[i] && !seqs[i])) { err = "apply edits: bad sequence"; return -1; }
        offs[i + 1] = offs[i] + lens[i];
    }
    if (n_edits && !edits) { err = "apply edits: bad arguments"; return -1; }
    if (check_edits(edits, n_edits, n_seqs, offs.data(), err)) return -1;
    HostText H;
    if (pack_host_text(T, Table::WS_REPAIR, n_seqs, seqs, lens, "apply edits", H, err)) return -1;
    return apply_checked(T, n_seqs, H.d_text, H.offs, edits, n_edits, out, err);
}

}  // namespace jk
