// polish_plan_check.cpp -- jasper_amd/csrc/polish_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_polish_plan_host.py).  No HIP, no GPU.
//
//   polish_plan_check FILE
//
// FILE holds tokens separated by blanks: commands, each a word and its numbers; the program prints the lines below per command
// and `ok` at the end.  Device addresses are made-up bases that are only added to; they are printed as offsets from their base.
//
//   layout k RM n len..                        -> "layout max_segs text_bound rec_bound aux_bound text_bytes pos_items cand_items flag_items cell_items"
//                                                 and per chunk "chunk cap off_text off_pos off_cand off_flag off_cell n_cells cand_cap"
//   forced n_chunks S                          -> "forced" and one 0/1 per chunk ("forced -" for an empty list); S = null, or "..." in quotes
//   geometry tmin cmin w m                     -> sets the geometry of the following `cuts` (without it: cut_geometry(k))
//   cuts k speculate n len.. ncand word.. per chunk: ncells cell..
//                                              -> per chunk "cuts pos chained pos chained .." and "sync 0/1 cells n" (want_sync, scan_cells)
//   table k RM tight n len.. ncand word.. per chunk: ncells cell..
//         nfail chunk.. text_bound rec_bound aux_bound          (bounds of the redo; -1: the layout's)
//                                              -> "table rc n_out tpos rpos apos", "first ..", per segment "seg <fields>" (print_seg);
//                                                 then the failed chunks unsegmented, behind the table: "redo rc n tpos rpos apos" and their "seg" lines
//   books n_chunks pass passes nseg, per segment: chunk status last len len0 own_lo own_hi0 seg_lo nrec naux lookups wrong
//                                              -> "books rc" and, rc != 0: "error <message>"; else per segment "b own_hi out_off idx_base seq_base rec_off aux_off",
//                                                 "newlen ..", "totals nrec naux lookups qv0 qv2", "qvchunk .." (the 0 and 2 entries per chunk)
//   chunks k RM pass passes n (len newlen)..   -> "chunks rc qv1 qv3" and "qvchunk .." (the 1 and 3 entries per chunk)
//   regroup n_chunks npass, per pass: auxhex nrec, per record: chunk pass seqno kind aux_off aux_len rep
//                                              -> per record in final order "rec chunk pass seqno kind aux_off", per chunk "aux hex"
#include "polish_plan.hpp"

#include <cstdio>
#include <fstream>

using namespace jk;

#define REQUIRE(x)                                                       \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);         \
            return 1;                                                    \
        }                                                                \
    } while (0)

static uint8_t *const TEXT = reinterpret_cast<uint8_t *>(0x100000000000ull), *const AUX = reinterpret_cast<uint8_t *>(0x200000000000ull),
                      *const CLS = reinterpret_cast<uint8_t *>(0x300000000000ull);
static FixRec *const RECS = reinterpret_cast<FixRec *>(0x400000000000ull);
static EditRec *const EDITS = reinterpret_cast<EditRec *>(0x500000000000ull);
static long long *const ARRIVE = reinterpret_cast<long long *>(0x600000000000ull);

static void print_seg(const SegDev &S) {
    // chunk first last chain_in seg_lo start_i stop_orig len0 len cap gs glen cls cls_n rec_cap edit_cap aux_cap own_lo own_hi own_hi0 buf recs edits aux arrive rest
    // (rest: the sum of every field the host leaves 0)
    uint64_t rest = (uint64_t)S.took_shortcut + S.nrec + S.naux + S.nedit + (uint64_t)S.status + (uint64_t)S.spec_fail + (uint64_t)S.wrong + S.lookups + S.ticks + (uint64_t)S.out_off;
    for (int q = 0; q < 12; ++q) rest += S.tk[q];
    std::printf("seg %u %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %u %u %u %lld %lld %lld %lld %lld %lld %lld %lld %llu\n", S.chunk, S.first, S.last, S.chain_in,
                (long long)S.seg_lo, (long long)S.start_i, (long long)S.stop_orig, (long long)S.len0, (long long)S.len, (long long)S.cap, (long long)S.gs, (long long)S.glen,
                S.cls ? (long long)(S.cls - CLS) : -1ll, (long long)S.cls_n, S.rec_cap, S.edit_cap, S.aux_cap, (long long)S.own_lo, (long long)S.own_hi, (long long)S.own_hi0,
                (long long)(S.buf - TEXT), (long long)(S.recs - RECS), (long long)(S.edits - EDITS), (long long)(S.aux - AUX), (long long)(S.arrive - ARRIVE), (unsigned long long)rest);
}

struct Batch {      // lengths, the unordered candidate words, the cells per chunk
    int n = 0;
    std::vector<int64_t> len, cells;
    std::vector<std::vector<int64_t>> cands, chunk_cells;
    bool read(std::istream &in) {
        in >> n;
        if (!in || n < 0) return false;
        len.resize((size_t)n);
        for (int64_t &l : len) in >> l;
        size_t nw = 0;
        in >> nw;
        std::vector<int64_t> words(nw);
        for (int64_t &w : words) in >> w;
        cands.resize((size_t)n);
        group_candidates(words.data(), nw, n, cands);
        chunk_cells.resize((size_t)n);
        for (auto &cc : chunk_cells) {
            size_t nc = 0;
            in >> nc;
            cc.resize(nc);
            for (int64_t &p : cc) in >> p;
        }
        return (bool)in;
    }
};

static int do_layout(std::istream &in) {
    int k = 0, n = 0;
    int64_t RM = 0;
    in >> k >> RM >> n;
    std::vector<int64_t> len((size_t)n);
    for (int64_t &l : len) in >> l;
    if (!in) return 2;
    const LaneLayout L = lane_layout(len.data(), n, k, RM);
    std::printf("layout %lld %zu %zu %zu %zu %zu %zu %zu %zu\n", (long long)L.max_segs, L.seg_text_bound, L.seg_rec_bound, L.seg_aux_bound, L.text_bytes, L.pos_items, L.cand_items,
                L.flag_items, L.cell_items);
    for (int c = 0; c < n; ++c)
        std::printf("chunk %lld %zu %zu %zu %zu %zu %u %u\n", (long long)L.cap[c], L.off_text[c], L.off_pos[c], L.off_cand[c], L.off_flag[c], L.off_cell[c], L.n_cells[c], L.cand_cap[c]);
    return 0;
}

static int do_forced(std::istream &in) {
    int n = 0;
    std::string s;
    in >> n >> s;
    if (!in) return 2;
    std::vector<char> f;
    if (s == "null") f = parse_forced_redo(nullptr, n);
    else {
        REQUIRE(s.size() >= 2 && s.front() == '"' && s.back() == '"');
        f = parse_forced_redo(s.substr(1, s.size() - 2).c_str(), n);
    }
    std::printf("forced");
    if (f.empty()) std::printf(" -");
    for (char x : f) std::printf(" %d", (int)x);
    std::printf("\n");
    return 0;
}

static int do_cuts(std::istream &in, const CutGeometry *geo) {
    int k = 0, speculate = 0;
    in >> k >> speculate;
    Batch B;
    if (!in || !B.read(in)) return 2;
    const CutGeometry g = geo ? *geo : cut_geometry(k);
    std::vector<Cut> cuts;
    for (int c = 0; c < B.n; ++c) {
        plan_cuts(B.cands[c], B.chunk_cells[c].data(), (uint32_t)B.chunk_cells[c].size(), B.len[c], k, g, speculate != 0, cuts);
        std::printf("cuts");
        for (const Cut &x : cuts) std::printf(" %lld %d", (long long)x.pos, (int)x.chained);
        std::printf("\nsync %d cells %u\n", (int)want_sync(B.len[c], k, g), scan_cells(1u << 30, B.len[c], k));
    }
    return 0;
}

static int do_table(std::istream &in) {
    int k = 0, tight = 0;
    int64_t RM = 0;
    in >> k >> RM >> tight;
    Batch B;
    if (!in || !B.read(in)) return 2;
    size_t nfail = 0;
    in >> nfail;
    std::vector<int> redo(nfail);
    for (int &c : redo) in >> c;
    long long tb = 0, rb = 0, ab = 0;
    in >> tb >> rb >> ab;
    if (!in) return 2;
    const LaneLayout L = lane_layout(B.len.data(), B.n, k, RM);
    for (int c = 0; c < B.n; ++c) {                      // the cells at their places in the batch's list
        REQUIRE(B.chunk_cells[c].size() == scan_cells(L.n_cells[c], B.len[c], k));
        B.cells.resize(L.cell_items, -7);
        std::copy(B.chunk_cells[c].begin(), B.chunk_cells[c].end(), B.cells.begin() + (long)L.off_cell[c]);
    }
    SegArena A;
    A.text = TEXT; A.recs = RECS; A.edits = EDITS; A.aux = AUX; A.arrive = ARRIVE;
    A.text_bound = L.seg_text_bound; A.rec_bound = L.seg_rec_bound; A.aux_bound = L.seg_aux_bound; A.max_segs = L.max_segs;
    const CutInput cin{B.len.data(), &B.cands, B.cells.data(), CLS, tight != 0};
    std::vector<int> all((size_t)B.n);
    for (int c = 0; c < B.n; ++c) all[(size_t)c] = c;
    std::vector<SegDev> segs((size_t)L.max_segs);
    std::vector<int32_t> first((size_t)B.n + 1, -1);
    size_t ns = 0;
    std::string err;
    int rc = build_segment_table(L, cin, all, true, A, segs.data(), ns, first.data(), err);
    std::printf("table %d %zu %zu %zu %zu\n", rc, ns, A.tpos, A.rpos, A.apos);
    if (rc) { std::printf("error %s\n", err.c_str()); return 0; }
    std::printf("first");
    for (int32_t f : first) std::printf(" %d", f);
    std::printf("\n");
    for (size_t s = 0; s < ns; ++s) print_seg(segs[s]);
    // the redo: behind the table, from the cursors it left
    SegArena behind = A;
    if (tb >= 0) behind.text_bound = (size_t)tb;
    if (rb >= 0) behind.rec_bound = (size_t)rb;
    if (ab >= 0) behind.aux_bound = (size_t)ab;
    std::vector<SegDev> again((size_t)L.max_segs);
    size_t nredo = 0;
    err.clear();
    rc = build_segment_table(L, cin, redo, false, behind, again.data(), nredo, nullptr, err);
    std::printf("redo %d %zu %zu %zu %zu\n", rc, nredo, behind.tpos, behind.rpos, behind.apos);
    REQUIRE((rc == 0) == err.empty() && (rc == 0 || (rc == -2 && err == "polish: internal segment arena bound exceeded")));
    for (size_t s = 0; s < nredo; ++s) print_seg(again[s]);
    return 0;
}

static int do_books(std::istream &in) {
    int n_chunks = 0, pass = 0, passes = 0;
    size_t ns = 0;
    in >> n_chunks >> pass >> passes >> ns;
    std::vector<SegDev> segs(ns);
    for (SegDev &S : segs) {
        memset(&S, 0, sizeof S);
        S.own_hi = -99;                                   // (what the device's summary may have left: not to be used)
        S.out_off = -99;
        in >> S.chunk >> S.status >> S.last >> S.len >> S.len0 >> S.own_lo >> S.own_hi0 >> S.seg_lo >> S.nrec >> S.naux >> S.lookups >> S.wrong;
    }
    if (!in) return 2;
    HostBooks B;
    PassCount P;
    P.reset(n_chunks);
    PolishOut R;
    R.reset(n_chunks);
    std::string err;
    const int rc = host_bookkeeping(segs, n_chunks, pass, passes, B, P, R, err);
    std::printf("books %d\n", rc);
    if (rc) { std::printf("error %s\n", err.c_str()); return 0; }
    for (size_t s = 0; s < ns; ++s)
        std::printf("b %lld %lld %lld %u %u %u\n", (long long)segs[s].own_hi, (long long)segs[s].out_off, (long long)B.idx_base[s], B.seq_base[s], B.rec_off[s], B.aux_off[s]);
    std::printf("newlen");
    for (int64_t v : P.newlen) std::printf(" %lld", (long long)v);
    std::printf("\ntotals %zu %zu %llu %lld %lld\nqvchunk", P.nrec, P.naux, (unsigned long long)R.lookups, (long long)R.qv[0], (long long)R.qv[2]);
    for (int c = 0; c < n_chunks; ++c) std::printf(" %lld %lld", (long long)R.qv_chunk[4 * (size_t)c], (long long)R.qv_chunk[4 * (size_t)c + 2]);
    std::printf("\n");
    REQUIRE(R.qv[1] == 0 && R.qv[3] == 0);
    return 0;
}

static int do_chunks(std::istream &in) {
    int k = 0, pass = 0, passes = 0, n = 0;
    int64_t RM = 0;
    in >> k >> RM >> pass >> passes >> n;
    std::vector<int64_t> len((size_t)n);
    PassCount P;
    P.reset(n);
    for (int c = 0; c < n; ++c) in >> len[(size_t)c] >> P.newlen[(size_t)c];
    if (!in) return 2;
    const LaneLayout L = lane_layout(len.data(), n, k, RM);
    PolishOut R;
    R.reset(n);
    std::string err;
    const int rc = account_chunks(len.data(), L, P, pass, passes, R, err);
    REQUIRE((rc == 0 && err.empty()) || (rc == -2 && err == "polish: chunk grew beyond its slack"));
    std::printf("chunks %d %lld %lld\nqvchunk", rc, (long long)R.qv[1], (long long)R.qv[3]);
    for (int c = 0; c < n; ++c) std::printf(" %lld %lld", (long long)R.qv_chunk[4 * (size_t)c + 1], (long long)R.qv_chunk[4 * (size_t)c + 3]);
    std::printf("\n");
    return 0;
}

static int do_regroup(std::istream &in) {
    int n_chunks = 0;
    size_t npass = 0;
    in >> n_chunks >> npass;
    PolishOut R;
    R.reset(n_chunks);
    std::vector<size_t> begin;
    std::vector<std::vector<uint8_t>> aux_pass(npass);
    for (size_t p = 0; p < npass; ++p) {
        std::string hex;
        size_t nrec = 0;
        in >> hex >> nrec;
        if (hex != "-")
            for (size_t i = 0; i + 1 < hex.size(); i += 2) aux_pass[p].push_back((uint8_t)std::stoi(hex.substr(i, 2), nullptr, 16));
        begin.push_back(R.recs.size());
        for (size_t i = 0; i < nrec; ++i) {
            FixRec f{};
            unsigned pass = 0, kind = 0;
            in >> f.chunk >> pass >> f.seqno >> kind >> f.aux_off >> f.aux_len >> f.rep;
            f.pass = (uint8_t)pass;
            f.kind = (uint8_t)kind;
            f.index = (int64_t)R.recs.size();
            R.recs.push_back(f);
        }
    }
    if (!in) return 2;
    regroup_and_sort(R, begin, aux_pass);
    for (const FixRec &f : R.recs) std::printf("rec %u %u %u %u %u\n", f.chunk, (unsigned)f.pass, f.seqno, (unsigned)f.kind, f.aux_off);
    for (const std::string &a : R.aux) {
        std::printf("aux ");
        if (a.empty()) std::printf("-");
        for (unsigned char ch : a) std::printf("%02x", ch);
        std::printf("\n");
    }
    return 0;
}

// the small pieces, on hand-made values
static int own_checks() {
    // summaries: ordinary only when no chunk has a bad segment or a failed speculation
    ChunkSummary s[3] = {{100, 2, 7, 1, 4, -1, 0}, {50, 0, 3, 0, 0, -1, 0}, {0, 1, 1, 2, 0, -1, 0}};
    REQUIRE(summaries_ordinary(s, 3) && summaries_ordinary(s, 0));
    s[1].spec_fail = 1;
    REQUIRE(!summaries_ordinary(s, 3) && summaries_ordinary(s, 1));
    s[1].spec_fail = 0;
    s[2].bad_seg = 0;
    REQUIRE(!summaries_ordinary(s, 3) && summaries_ordinary(s, 2));
    PolishOut R;
    R.reset(3);
    PassCount P;
    P.reset(3);
    account_summaries(s, 3, 0, 0, P, R);               // pass 0 of 0 fixing passes: first and last at once
    REQUIRE(P.newlen[0] == 100 && P.newlen[1] == 50 && P.newlen[2] == 0 && P.nrec == 3 && P.naux == 4 && R.lookups == 11);
    REQUIRE(R.qv[0] == 3 && R.qv[2] == 3 && R.qv_chunk[0] == 2 && R.qv_chunk[2] == 2 && R.qv_chunk[8] == 1 && R.qv_chunk[4] == 0);
    account_summaries(s, 3, 1, 2, P, R);               // a middle pass counts no wrong k-mers
    REQUIRE(R.qv[0] == 3 && R.qv[2] == 3 && R.lookups == 22 && P.nrec == 6);
    // the redo list and the merged table
    std::vector<SegDev> segs(5);
    for (SegDev &S : segs) memset(&S, 0, sizeof S);
    const uint32_t chunk[5] = {0, 0, 1, 2, 2};
    const int64_t lo[5] = {0, 500, 0, 0, 900};
    for (int i = 0; i < 5; ++i) { segs[(size_t)i].chunk = chunk[i]; segs[(size_t)i].seg_lo = lo[i]; segs[(size_t)i].wrong = i; }
    segs[1].spec_fail = 1;
    segs[2].spec_fail = 1;
    segs[2].status = PS_REC_OVERFLOW;                   // (a segment that failed otherwise is the bookkeeping's, not the redo's)
    std::vector<char> failed;
    REQUIRE(chunks_to_redo(segs, {}, 3, failed) == std::vector<int>({0}) && failed == std::vector<char>({1, 0, 0}));
    REQUIRE(chunks_to_redo(segs, {0, 0, 1}, 3, failed) == std::vector<int>({0, 2}));
    segs[1].spec_fail = 0;
    REQUIRE(chunks_to_redo(segs, {}, 3, failed).empty());
    chunks_to_redo(segs, {1, 0, 1}, 3, failed);
    std::vector<SegDev> again(2);
    for (SegDev &S : again) memset(&S, 0, sizeof S);
    again[0].chunk = 0; again[0].wrong = 70;
    again[1].chunk = 2; again[1].wrong = 72;
    merge_redo(segs, failed, again);
    REQUIRE(segs.size() == 3 && segs[0].wrong == 70 && segs[1].chunk == 1 && segs[1].wrong == 2 && segs[2].wrong == 72);
    // the comparator
    FixRec a{}, b{};
    a.chunk = 1; b.chunk = 1; a.pass = 0; b.pass = 1; a.seqno = 9; b.seqno = 0;
    REQUIRE(fixrec_less(a, b) && !fixrec_less(b, a) && !fixrec_less(a, a));
    b.pass = 0;
    REQUIRE(fixrec_less(b, a));
    b.chunk = 0; b.pass = 5;
    REQUIRE(fixrec_less(b, a));
    REQUIRE(al256(0) == 0 && al256(1) == 256 && al256(256) == 256 && al256(257) == 512);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: polish_plan_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string cmd;
    CutGeometry geo{};
    bool have_geo = false;
    while (in >> cmd) {
        int rc = 2;
        if (cmd == "layout") rc = do_layout(in);
        else if (cmd == "forced") rc = do_forced(in);
        else if (cmd == "geometry") { in >> geo.tmin >> geo.cmin >> geo.w >> geo.m; geo.clean_cell = CLEAN_CELL; have_geo = true; rc = in ? 0 : 2; }
        else if (cmd == "cuts") rc = do_cuts(in, have_geo ? &geo : nullptr);
        else if (cmd == "table") rc = do_table(in);
        else if (cmd == "books") rc = do_books(in);
        else if (cmd == "chunks") rc = do_chunks(in);
        else if (cmd == "regroup") rc = do_regroup(in);
        if (rc) {
            std::fprintf(stderr, "command %s: %d\n", cmd.c_str(), rc);
            return rc;
        }
    }
    if (own_checks()) return 1;
    std::printf("ok\n");
    return 0;
}
