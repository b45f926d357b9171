// polish_plan.hpp -- everything a polishing lane (polish_host.hip) computes on the host: the layout of its arenas, where a pass cuts
// a chunk, the segment table, the bookkeeping after the walks, the order of the records.  Plain C++: no HIP call, no getenv; device
// addresses come in as base pointers that are only added to, never dereferenced.  tools/polish_plan_check.cpp builds it stand-alone
// under sanitizers (tests/test_polish_plan_host.py).
#pragma once
#include "polish_types.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace jk {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the result of a call ---------------------------------------------------------------------------------------------------------
struct PolishOut {
    std::vector<std::string> seqs;   // polished chunk texts, batch order (empty strings while the text is kept in HBM)
    std::vector<const uint8_t *> d_seqs;   // keep_on_device: where each polished chunk lies in the table's workspace
    std::vector<int64_t> d_lens;
    std::vector<FixRec> recs;        // ordered by chunk, pass, emission; index in chunk coordinates
    std::vector<std::string> aux;    // per chunk: bytes referenced by its 'x' records
    int64_t qv[4];                   // bad0, total0, badP, totalP   (src/jasper.py:107-111)
    std::vector<int64_t> qv_chunk;   // the same four per chunk record (4 * n_chunks): callers that group chunks into files
    uint64_t lookups;
    double seconds;                  // device time of all passes (HIP events on the table's stream)
    uint64_t n_segments;             // segments walked (all passes)
    uint64_t n_respeculated;         // chunks redone unsegmented because a segment's assumption did not hold

    void reset(int n_chunks) {       // empty results for n_chunks chunk records
        seqs.assign(n_chunks, std::string());
        d_seqs.clear();
        d_lens.clear();
        aux.assign(n_chunks, std::string());
        recs.clear();
        qv[0] = qv[1] = qv[2] = qv[3] = 0;
        qv_chunk.assign((size_t)4 * n_chunks, 0);
        lookups = 0;
        seconds = 0;
        n_segments = 0;
        n_respeculated = 0;
    }
};

// records: by chunk, pass, emission
inline bool fixrec_less(const FixRec &a, const FixRec &b) {
    if (a.chunk != b.chunk) return a.chunk < b.chunk;
    if (a.pass != b.pass) return a.pass < b.pass;
    return a.seqno < b.seqno;
}
inline void sort_records(std::vector<FixRec> &recs) { std::stable_sort(recs.begin(), recs.end(), fixrec_less); }

// ---- layout -------------------------------------------------------------------------------------------------------------------------
// Every slack / bound is a guess about how much a pass can add; RM = 1 is generous for real polishing (edits are ~0.1 % of the
// text), RM = 8 is the repeat of a call that exceeded one.
struct LaneLayout {
    int n_chunks = 0, k = 0;
    int64_t RM = 1;
    CutGeometry geo{};
    std::vector<int64_t> cap;                                                // bytes a chunk's text may grow to
    std::vector<size_t> off_text, off_pos, off_cand, off_flag, off_cell;     // a chunk's place in the text arenas, classes, candidates, flags, cells
    std::vector<uint32_t> n_cells, cand_cap;
    size_t text_bytes = 0, pos_items = 0, cand_items = 0, flag_items = 0, cell_items = 0;
    size_t seg_text_bound = 0, seg_rec_bound = 0, seg_aux_bound = 0;         // the three segment arenas: bytes, records, bytes
    int64_t max_segs = 0;
};
inline LaneLayout lane_layout(const int64_t *lens, int n_chunks, int k, int64_t RM) {
    LaneLayout L;
    L.n_chunks = n_chunks;
    L.k = k;
    L.RM = RM;
    L.geo = cut_geometry(k);
    const size_t n = (size_t)std::max(n_chunks, 0);
    L.cap.resize(n);
    L.off_text.resize(n); L.off_pos.resize(n); L.off_cand.resize(n); L.off_flag.resize(n); L.off_cell.resize(n);
    L.n_cells.resize(n); L.cand_cap.resize(n);
    for (size_t c = 0; c < n; ++c) {
        const int64_t cap = lens[c] + RM * std::max<int64_t>(4096, lens[c] / 8) + 64;
        L.cap[c] = cap;
        L.off_text[c] = L.text_bytes;  L.text_bytes += al256((size_t)cap);
        L.off_pos[c] = L.pos_items;    L.pos_items += al256((size_t)cap);
        L.cand_cap[c] = (uint32_t)std::min<int64_t>(1 << 28, cap / (4 * k) + 16);
        L.off_cand[c] = L.cand_items;  L.cand_items += L.cand_cap[c];
        L.off_flag[c] = L.flag_items;  L.flag_items += al256((size_t)(cap >> 6) + 2);
        L.n_cells[c] = (uint32_t)(cap / CLEAN_CELL + 1);
        L.off_cell[c] = L.cell_items;  L.cell_items += L.n_cells[c];
        const int64_t ms = cap / L.geo.tmin + 2;
        L.max_segs += ms;
        const int64_t tb = cap + ms * (L.geo.w + L.geo.m + 64);
        L.seg_text_bound += (size_t)(tb + RM * (tb / 8 + ms * 1280));
        L.seg_rec_bound += (size_t)(RM * (2 * tb / k + 16 * ms));
        L.seg_aux_bound += (size_t)(RM * (2 * tb + 1024 * ms));
    }
    return L;
}

// tests: the chunks (lane-local indices, or "all") that JASPER_POLISH_TEST_REDO lists; empty when it lists nothing
inline std::vector<char> parse_forced_redo(const char *s, int n_chunks) {
    std::vector<char> forced;
    if (!s || !*s) return forced;
    const bool all = strcmp(s, "all") == 0;
    forced.assign((size_t)std::max(n_chunks, 0), (char)all);
    for (const char *p = s; *p && !forced.empty() && !all;) {
        char *e = nullptr;
        const long c = strtol(p, &e, 10);
        if (e == p) break;
        if (c >= 0 && c < n_chunks) forced[(size_t)c] = 1;
        p = *e == ',' ? e + 1 : e;
    }
    return forced;
}

// ---- where a pass cuts a chunk --------------------------------------------------------------------------------------------------------
// the scan looks for sync points only in a chunk that two segments of TMIN fit into
inline bool want_sync(int64_t len, int k, const CutGeometry &g) { return (len - k + 1) > 2 * g.tmin; }
// clean-zone cells the scan fills for a chunk of `len` bases (of the n_cells its arena has)
inline uint32_t scan_cells(uint32_t n_cells, int64_t len, int k) {
    return (uint32_t)std::min<int64_t>(n_cells, std::max<int64_t>(0, len - k + 1) / CLEAN_CELL + 1);
}

// the batch's unordered candidate words (chunk << 40) | pos into one list per chunk
inline void group_candidates(const int64_t *words, size_t n, int n_chunks, std::vector<std::vector<int64_t>> &per_chunk) {
    for (int c = 0; c < n_chunks; ++c) per_chunk[c].clear();
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = words[i];
        const int64_t c = v >> 40;
        if (c >= 0 && c < n_chunks) per_chunk[c].push_back(v & ((1ll << 40) - 1));
    }
}

struct Cut {
    int64_t pos;       // chunk coordinate of the cut
    char chained;      // a clean-zone boundary: the segment to its right starts where its left neighbour's walk arrives
};
// One chunk's cuts, in text order.  Sync points: the candidates at least TMIN from the last one kept, from the chunk start and from
// the chunk end.  Then clean-zone boundaries (cells[g] or -1, n_cells of them) inside the stretches the sync points leave long:
// at least CMIN from both neighbours.
inline void plan_cuts(const std::vector<int64_t> &cands, const int64_t *cells, uint32_t n_cells, int64_t len, int k, const CutGeometry &g, bool speculate,
                      std::vector<Cut> &out) {
    out.clear();
    if (!speculate) return;
    if (want_sync(len, k, g) && !cands.empty()) {
        std::vector<int64_t> sorted = cands;
        std::sort(sorted.begin(), sorted.end());
        int64_t last = 0;
        for (int64_t p : sorted)
            if (p - last >= g.tmin && len - p >= g.tmin) { out.push_back(Cut{p, 0}); last = p; }
    }
    if (len - k + 1 > 2 * g.cmin) {
        std::vector<Cut> merged;
        size_t si = 0;
        int64_t last = 0;
        for (uint32_t c = 0; c <= n_cells; ++c) {
            const int64_t p = c < n_cells ? cells[c] : INT64_MAX;
            while (si < out.size() && out[si].pos <= p) { merged.push_back(out[si]); last = out[si].pos; ++si; }
            if (c == n_cells || p < 0) continue;
            const int64_t next = si < out.size() ? out[si].pos : len;
            if (p - last >= g.cmin && next - p >= g.cmin) { merged.push_back(Cut{p, 1}); last = p; }
        }
        out.swap(merged);
    }
}

// ---- the segment table ----------------------------------------------------------------------------------------------------------------
// the three arenas segments take their buffers from, and the arrive slots; cursors run on from table to table (the redo places its
// segments behind the first table's) until rewind()
struct SegArena {
    uint8_t *text = nullptr;
    FixRec *recs = nullptr;
    EditRec *edits = nullptr;          // one edit list entry per possible record
    uint8_t *aux = nullptr;
    long long *arrive = nullptr;
    size_t text_bound = 0, rec_bound = 0, aux_bound = 0;
    int64_t max_segs = 0;
    size_t tpos = 0, rpos = 0, apos = 0;

    void rewind() { tpos = rpos = apos = 0; }
    bool fits() const { return tpos <= text_bound && rpos <= rec_bound && apos <= aux_bound; }
    void place(SegDev &S) {            // needs cap, rec_cap, aux_cap
        S.buf = text + tpos;           tpos += al256((size_t)S.cap);
        S.recs = recs + rpos;
        S.edits = edits + rpos;
        S.edit_cap = S.rec_cap;        rpos += S.rec_cap;
        S.aux = aux + apos;            apos += al256(S.aux_cap);
    }
};
inline const char *arena_exceeded() { return "polish: internal segment arena bound exceeded"; }

// the cuts.size() + 1 segments of chunk c (polish_types.hpp has the formulas) into out[n_out ..]; cls = the chunk's classes
inline int fill_chunk(int c, int64_t len, const std::vector<Cut> &cuts, const uint8_t *cls, int k, const CutGeometry &g, int64_t RM, bool tight, SegArena &A,
                      SegDev *out, size_t &n_out, std::string &err) {
    const int m = (int)cuts.size();
    if ((int64_t)n_out + m + 1 > A.max_segs) { err = arena_exceeded(); return -2; }
    for (int j = 0; j <= m; ++j) {
        SegDev &S = out[n_out++];
        memset(&S, 0, sizeof S);
        S.chunk = (uint32_t)c;
        S.first = (j == 0);
        S.last = (j == m);
        S.seg_lo = j == 0 ? 0 : cuts[j - 1].pos - g.w;
        S.start_i = j == 0 ? 0 : g.w;
        S.chain_in = j > 0 && cuts[j - 1].chained;
        S.arrive = A.arrive + n_out;             // (= 1 + its index; slot 0 is never read: a first segment is not chained)
        S.stop_orig = j == m ? INT64_MAX : cuts[j].pos;
        const int64_t seg_hi = j == m ? len : std::min<int64_t>(len, cuts[j].pos + g.m);
        S.len0 = seg_hi - S.seg_lo;
        S.len = S.len0;
        S.cap = S.len0 + (tight ? 2 : RM * std::max<int64_t>(1024, S.len0 / 8));
        S.gs = 0;
        S.glen = S.cap - S.len0;
        S.cls = (len - k + 1 > 0) ? cls : nullptr;
        S.cls_n = std::max<int64_t>(0, len - k + 1);
        S.rec_cap = (uint32_t)std::min<int64_t>(0x7fffffff, RM * (2 * S.len0 / k + 16));
        S.aux_cap = (uint32_t)std::min<int64_t>(0x7fffffff, RM * (2 * S.len0 + 1024));
        A.place(S);
        // owned part of the text: chunk coordinates [B_j, B_{j+1}), B = cut - 2k
        S.own_lo = j == 0 ? 0 : 2ll * k;                   // local (no edit can precede it)
        S.own_hi = j == m ? -1 : (cuts[j].pos - 2ll * k) - S.seg_lo;   // local, before adding this segment's delta
        S.own_hi0 = S.own_hi;
    }
    return 0;
}

// what a pass's cut needs of the lane: the current lengths, the fetched candidates and cells, where the classes lie
struct CutInput {
    const int64_t *len = nullptr;
    const std::vector<std::vector<int64_t>> *cands = nullptr;   // per chunk, unordered
    const int64_t *cells = nullptr;                             // all chunks' clean-zone cells (LaneLayout::off_cell)
    uint8_t *cls = nullptr;                                     // base of the class array the pass reads (LaneLayout::off_pos)
    bool tight = false;                                         // tests: segments with two bytes of slack
};
// segments of `chunks` into out[0 .. n_out) (room for max_segs), buffers from A's cursors on; first_of (optional): first_of[i] =
// index of chunks[i]'s first segment.  -2 when the table or an arena does not hold them.
inline int build_segment_table(const LaneLayout &L, const CutInput &in, const std::vector<int> &chunks, bool speculate, SegArena &A, SegDev *out, size_t &n_out,
                               int32_t *first_of, std::string &err) {
    n_out = 0;
    size_t ci = 0;
    std::vector<Cut> cuts;
    for (int c : chunks) {
        if (first_of) first_of[ci++] = (int32_t)n_out;
        const int64_t len = in.len[c];
        plan_cuts((*in.cands)[c], in.cells + L.off_cell[c], scan_cells(L.n_cells[c], len, L.k), len, L.k, L.geo, speculate, cuts);
        if (const int rc = fill_chunk(c, len, cuts, in.cls + L.off_pos[c], L.k, L.geo, L.RM, in.tight, A, out, n_out, err)) return rc;
    }
    if (first_of) first_of[ci] = (int32_t)n_out;
    if (!A.fits() || (int64_t)n_out > A.max_segs) { err = arena_exceeded(); return -2; }
    return 0;
}

// ---- after the walks --------------------------------------------------------------------------------------------------------------------
// what a pass adds up, whoever does the bookkeeping
struct PassCount {
    std::vector<int64_t> newlen;     // per chunk: length of the stitched text
    size_t nrec = 0, naux = 0;       // fix records / aux bytes of the pass
    void reset(int n_chunks) { newlen.assign((size_t)n_chunks, 0); nrec = naux = 0; }
};
inline void count_wrong(PolishOut &R, int c, int pass, int passes, int64_t wrong) {
    if (pass == 0) { R.qv[0] += wrong; R.qv_chunk[4 * (size_t)c + 0] += wrong; }
    if (pass == passes) { R.qv[2] += wrong; R.qv_chunk[4 * (size_t)c + 2] += wrong; }
}

// the ordinary path: the device did the bookkeeping (seg_summary_kernel), nothing failed
inline bool summaries_ordinary(const ChunkSummary *sum, int n_chunks) {
    for (int c = 0; c < n_chunks; ++c)
        if (!(sum[c].bad_seg < 0 && !sum[c].spec_fail)) return false;
    return true;
}
inline void account_summaries(const ChunkSummary *sum, int n_chunks, int pass, int passes, PassCount &P, PolishOut &R) {
    for (int c = 0; c < n_chunks; ++c) {
        const ChunkSummary &S = sum[c];
        P.newlen[c] = S.newlen;
        P.nrec += S.nrec;
        P.naux += S.naux;
        R.lookups += S.lookups;
        count_wrong(R, c, pass, passes, S.wrong);
    }
}

// the rare path.  Chunks to redo unsegmented: a segment's speculation failed, or the tests force it
inline std::vector<int> chunks_to_redo(const std::vector<SegDev> &segs, const std::vector<char> &forced, int n_chunks, std::vector<char> &failed) {
    failed.assign((size_t)n_chunks, 0);
    for (const SegDev &S : segs)
        if (S.spec_fail && S.status == PS_OK) failed[S.chunk] = 1;
    for (size_t c = 0; c < forced.size(); ++c)
        if (forced[c]) failed[c] = 1;
    std::vector<int> redo;
    for (int c = 0; c < n_chunks; ++c) if (failed[c]) redo.push_back(c);
    return redo;
}
// the table after a redo: the segments of the chunks that held, and the redone chunks' single segments, in chunk and text order
inline void merge_redo(std::vector<SegDev> &segs, const std::vector<char> &failed, const std::vector<SegDev> &redo_segs) {
    std::vector<SegDev> good;
    for (const SegDev &S : segs) if (!failed[S.chunk]) good.push_back(S);
    segs.swap(good);
    segs.insert(segs.end(), redo_segs.begin(), redo_segs.end());
    std::stable_sort(segs.begin(), segs.end(), [](const SegDev &a, const SegDev &b) { return a.chunk != b.chunk ? a.chunk < b.chunk : a.seg_lo < b.seg_lo; });
}

inline const char *polish_status_name(int status) {
    static const char *names[] = {"ok", "text grew beyond its slack", "fix-record buffer overflow", "aux buffer overflow",
                                  "path-extension scratch exhausted", "reference IndexError (src/jasper.py:221)",
                                  "trial string too long"};
    return names[status];
}
// The host twin of seg_summary_kernel + seg_offsets_kernel, on the whole table (a chunk's segments consecutive, in text order):
// own_hi / out_off of every segment, the four coordinate bases the gather needs, the pass's counts.  A segment that did not end
// PS_OK fails the call: -4 when the reference itself would exit 1, else -2 (capacity: the caller repeats with more room).
struct HostBooks {
    std::vector<int64_t> idx_base;
    std::vector<uint32_t> seq_base, rec_off, aux_off;
};
inline int host_bookkeeping(std::vector<SegDev> &segs, int n_chunks, int pass, int passes, HostBooks &B, PassCount &P, PolishOut &R, std::string &err) {
    const size_t ns = segs.size();
    B.idx_base.assign(ns, 0);
    B.seq_base.assign(ns, 0); B.rec_off.assign(ns, 0); B.aux_off.assign(ns, 0);
    std::vector<int64_t> shift((size_t)n_chunks, 0);
    std::vector<uint32_t> seqc((size_t)n_chunks, 0);
    for (size_t s = 0; s < ns; ++s) {
        SegDev &S = segs[s];
        const int c = (int)S.chunk;
        if (S.status != PS_OK) {
            err = std::string("polish: chunk ") + std::to_string(c) + ": " + polish_status_name(S.status);
            return S.status == PS_REF_INDEXERROR ? -4 : -2;
        }
        const int64_t d = S.len - S.len0;
        S.own_hi = S.last ? S.len : S.own_hi0 + d;        // (from own_hi0: the device's summary pass may have written own_hi already)
        S.out_off = P.newlen[c];
        P.newlen[c] += S.own_hi - S.own_lo;
        B.idx_base[s] = S.seg_lo + shift[c];
        shift[c] += d;
        B.seq_base[s] = seqc[c];
        seqc[c] += S.nrec;
        B.rec_off[s] = (uint32_t)P.nrec;
        B.aux_off[s] = (uint32_t)P.naux;
        P.nrec += S.nrec;
        P.naux += S.naux;
        R.lookups += S.lookups;
        count_wrong(R, c, pass, passes, S.wrong);
    }
    return 0;
}

// both paths: the k-mers of the pass (src/jasper.py:51,107-111), and no chunk may have outgrown its arena place
inline int account_chunks(const int64_t *len, const LaneLayout &L, const PassCount &P, int pass, int passes, PolishOut &R, std::string &err) {
    int rc = 0;
    for (int c = 0; c < L.n_chunks; ++c) {
        if (pass == 0) { R.qv[1] += len[c] - L.k + 1; R.qv_chunk[4 * (size_t)c + 1] += len[c] - L.k + 1; }
        if (pass == passes) { R.qv[3] += len[c] - L.k + 1; R.qv_chunk[4 * (size_t)c + 3] += len[c] - L.k + 1; }
        if (P.newlen[c] > L.cap[c]) { err = "polish: chunk grew beyond its slack"; rc = -2; }
    }
    return rc;
}

// ---- end of call ----------------------------------------------------------------------------------------------------------------------
// The aux bytes of 'x' records, gathered per pass (aux_pass[p] belongs to the records from rec_pass_begin[p] on), regrouped per
// chunk in pass and emission order; aux_off becomes the offset in the chunk's bytes.  Then the records in their final order.
inline void regroup_and_sort(PolishOut &R, const std::vector<size_t> &rec_pass_begin, const std::vector<std::vector<uint8_t>> &aux_pass) {
    for (size_t p = 0; p < rec_pass_begin.size(); ++p) {
        const size_t b = rec_pass_begin[p], e = p + 1 < rec_pass_begin.size() ? rec_pass_begin[p + 1] : R.recs.size();
        for (size_t i = b; i < e; ++i) {
            FixRec &f = R.recs[i];
            if (f.kind == 'x') {
                std::string &a = R.aux[f.chunk];
                const size_t n = (size_t)f.aux_len + f.rep;
                const uint32_t no = (uint32_t)a.size();
                a.append(reinterpret_cast<const char *>(aux_pass[p].data()) + f.aux_off, n);
                f.aux_off = no;
            }
        }
    }
    sort_records(R.recs);
}

}  // namespace jk
