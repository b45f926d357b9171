// repair_host_check.cpp -- the host side of the repair stage (jasper_amd/csrc/repair_host.hpp: normalise, select, check, plan) as a
// stand-alone program, for a sanitizer build on a machine without a GPU:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I jasper_amd/csrc tools/repair_host_check.cpp -o /tmp/rp_check && /tmp/rp_check
// Prints `ok` and exits 0, or says what differs and exits 1.
#include "repair_host.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace jk;

static Edit ed(uint32_t seq, int64_t pos, uint32_t rlen, const std::string &y, uint32_t amin = 5, int source = ES_COMPOUND) {
    Edit e = edit_make(seq, pos, rlen, 0, amin, source);
    for (char ch : y) edit_push(e, (unsigned)(std::strchr("ACGT", ch) - "ACGT"));
    return e;
}
static std::string str(const Edit &e) {
    std::string y;
    for (int i = 0; i < (int)e.len; ++i) y += "ACGT"[edit_base(e, i)];
    return y;
}
// the records' shapes, as the scans' headers have them (only the fields normalisation reads)
struct V { int64_t pos; uint32_t seq, ref_min, alt_min; uint8_t ref, alt, kind, pad; };
struct I { int64_t pos; uint32_t seq, ref_min, alt_min; uint16_t len; uint8_t type, base, kind; };
struct M { int64_t pos; uint32_t seq, ref_min, alt_min, bases; uint16_t len; uint8_t kind; };
struct Cp { int64_t pos; uint32_t seq, ref_min, alt_min, ref_len; uint64_t bases[2]; uint16_t len; };

// the selection's rule applied pair by pair
static bool conflict(const Edit &a, const Edit &b, int k) {
    if (a.seq != b.seq) return false;
    const bool ab = a.pos != b.pos ? a.pos < b.pos : edit_end(a) <= edit_end(b);
    const Edit &x = ab ? a : b, &y = ab ? b : a;
    return y.pos - edit_end(x) < k - 1;
}

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main() {
    std::string err;
    // normalisation: error records only, one shape
    {
        std::vector<V> vs = {{10, 0, 0, 7, 'A', 'G', 2, 0}, {20, 0, 9, 7, 'A', 'C', 1, 0}};
        std::vector<I> is = {{30, 1, 1, 6, 3, 1, 'T', 2}, {40, 1, 0, 5, 2, 2, 'C', 2}, {50, 1, 8, 5, 1, 1, 'A', 1}};
        std::vector<M> ms = {{60, 0, 0, 4, 0x1Bu, 4, 2}, {70, 0, 7, 4, 0x1u, 2, 1}};      // 0x1B = T G C A from the low pair up
        std::vector<Cp> cs = {{80, 2, 1, 3, 5, {0x24u, 0}, 3}};                           // A C G
        std::vector<Edit> e;
        CHECK(!edits_from_variants(vs, e, err) && !edits_from_indels(is, e, err) && !edits_from_mixed(ms, e, err) && !edits_from_compound(cs, e, err));
        CHECK(e.size() == 5);
        CHECK(e[0].source == ES_SUB && e[0].pos == 10 && e[0].ref_len == 1 && str(e[0]) == "G" && e[0].alt_min == 7);
        CHECK(e[1].source == ES_INS && e[1].pos == 30 && e[1].ref_len == 0 && str(e[1]) == "TTT" && e[1].seq == 1);
        CHECK(e[2].source == ES_DEL && e[2].pos == 40 && e[2].ref_len == 2 && str(e[2]).empty());
        CHECK(e[3].source == ES_MIXED && e[3].ref_len == 0 && str(e[3]) == "TGCA");
        CHECK(e[4].source == ES_COMPOUND && e[4].ref_len == 5 && str(e[4]) == "ACG" && e[4].seq == 2);
        std::vector<V> bad = {{10, 0, 0, 7, 'A', 'N', 2, 0}};
        CHECK(edits_from_variants(bad, e, err) == -1);
    }
    const int k = 5;                                    // edits conflict when fewer than 4 bytes lie between them
    Selection S;
    // priority: the shorter edit first, then the larger alt_min; a chain a - b - c where b loses to both and a, c are far enough apart
    {
        std::vector<Edit> e = {ed(0, 100, 1, "G", 5, ES_SUB), ed(0, 103, 3, "ACG", 9), ed(0, 109, 1, "T", 5, ES_SUB), ed(0, 200, 2, "AC", 3), ed(0, 203, 2, "GT", 4)};
        select_edits(e, k, S);
        CHECK(S.records == 5 && S.conflicts == 2 && S.ambiguous == 0 && S.accepted.size() == 3);
        CHECK(S.accepted[0].pos == 100 && S.accepted[1].pos == 109 && S.accepted[2].pos == 203);
    }
    // exactly k - 1 bytes apart is no conflict, one less is; an insertion has q = pos
    {
        std::vector<Edit> e = {ed(0, 10, 1, "A"), ed(0, 15, 0, "CC"), ed(0, 19, 2, ""), ed(0, 24, 1, "T")};      // 15 - 11 = 4; 19 - 15 = 4; 24 - 21 = 3
        select_edits(e, k, S);
        CHECK(S.accepted.size() == 3 && S.conflicts == 1 && S.accepted[2].pos == 19);
    }
    // nesting: a long edit around a short one loses to it, and an edit equal in (pos, q) conflicts too
    {
        std::vector<Edit> e = {ed(0, 50, 20, "ACGTACGTAC"), ed(0, 58, 1, "G", 5, ES_SUB), ed(0, 58, 1, "GA", 5)};
        select_edits(e, k, S);
        CHECK(S.accepted.size() == 1 && S.accepted[0].source == ES_SUB && S.conflicts == 2);
    }
    // ambiguity: the same place, lengths and alt_min, another y -- both go; a third with another alt_min stays.  A duplicate is one edit.
    {
        std::vector<Edit> e = {ed(0, 30, 2, "AC", 5), ed(0, 30, 2, "AG", 5), ed(0, 30, 2, "TT", 6), ed(1, 30, 2, "AC", 5), ed(1, 30, 2, "AC", 5, ES_MIXED)};
        select_edits(e, k, S);
        CHECK(S.records == 4 && S.ambiguous == 2 && S.conflicts == 0 && S.accepted.size() == 2);
        CHECK(str(S.accepted[0]) == "TT" && S.accepted[1].seq == 1 && S.accepted[1].source == ES_MIXED);      // (sources in ascending order: mixed = 4 before compound = 5)
    }
    // two sequences do not see each other
    {
        std::vector<Edit> e = {ed(0, 10, 1, "A"), ed(1, 10, 1, "A"), ed(1, 11, 1, "C"), ed(2, 0, 0, "G")};
        select_edits(e, k, S);
        CHECK(S.accepted.size() == 3 && S.conflicts == 1 && S.accepted[0].seq == 0 && S.accepted[1].seq == 1 && S.accepted[1].pos == 10 && S.accepted[2].seq == 2);
    }
    // many: what is accepted is conflict-free pair by pair, and every edit that was left out conflicts with an accepted one or is ambiguous
    {
        std::mt19937_64 rng(11);
        for (int it = 0; it < 50; ++it) {
            std::vector<Edit> e;
            const int n = 1 + (int)(rng() % 120);
            for (int i = 0; i < n; ++i) {
                std::string y(rng() % 5, 'A');
                for (char &ch : y) ch = "ACGT"[rng() % 4];
                const uint32_t rlen = (uint32_t)(rng() % 4);
                if (y.empty() && !rlen) y = "C";
                e.push_back(ed((uint32_t)(rng() % 3), (int64_t)(rng() % 300), rlen, y, 3 + (uint32_t)(rng() % 4)));
            }
            std::vector<Edit> all = e;
            const int kk = 2 + (int)(rng() % 9);
            select_edits(e, kk, S);
            CHECK(S.records == S.accepted.size() + S.conflicts + S.ambiguous && S.records <= all.size() && !S.accepted.empty());
            for (size_t a = 0; a < S.accepted.size(); ++a)
                for (size_t b = a + 1; b < S.accepted.size(); ++b) CHECK(!conflict(S.accepted[a], S.accepted[b], kk));
            uint64_t out = 0;
            for (const Edit &x : e) {                   // (e: the list without duplicates)
                bool in = false, clash = false, tie = false;
                for (const Edit &a : S.accepted) in = in || (a.seq == x.seq && a.pos == x.pos && a.ref_len == x.ref_len && a.len == x.len && !edit_cmp_y(a, x));
                for (const Edit &a : S.accepted) clash = clash || conflict(a, x, kk);
                for (const Edit &o : e) tie = tie || (o.seq == x.seq && o.pos == x.pos && o.ref_len == x.ref_len && o.len == x.len && o.alt_min == x.alt_min && edit_cmp_y(o, x));
                CHECK(in || clash || tie);
                out += !in;
            }
            CHECK(out == S.conflicts + S.ambiguous);
            // the accepted list passes the check of what apply may get, in sequences long enough for it
            const int64_t offs[4] = {0, 400, 800, 1200};
            CHECK(check_edits(S.accepted.data(), S.accepted.size(), 3, offs, err) == 0);
        }
    }
    // the plan: output positions, offsets, int64 throughout
    {
        const int64_t offs[4] = {0, 100, 100, 5000000000ll};      // sequence 1 is empty
        std::vector<Edit> e = {ed(0, 0, 0, "ACG"), ed(0, 10, 4, ""), ed(0, 99, 1, "TT"), ed(2, 0, 1, "C"), ed(2, 4899999999ll, 1, "")};
        CHECK(check_edits(e.data(), e.size(), 3, offs, err) == 0);
        EditPlan P;
        plan_edits(e.data(), e.size(), 3, offs, P);
        const int64_t src[5] = {0, 10, 99, 100, 4900000099ll}, dst[5] = {0, 13, 98, 100, 4900000099ll};
        for (int i = 0; i < 5; ++i) CHECK(P.src[i] == src[i] && P.dst[i] == dst[i]);
        CHECK(P.new_offsets[0] == 0 && P.new_offsets[1] == 100 && P.new_offsets[2] == 100 && P.new_offsets[3] == 4999999999ll);
        plan_edits(nullptr, 0, 3, offs, P);
        CHECK(P.src.empty() && P.new_offsets[3] == offs[3]);
        const int64_t shifted[3] = {7, 17, 27};         // a text that does not start at 0: positions count from its first byte
        std::vector<Edit> f = {ed(1, 2, 0, "A")};
        plan_edits(f.data(), 1, 2, shifted, P);
        CHECK(P.src[0] == 12 && P.dst[0] == 12 && P.new_offsets[0] == 0 && P.new_offsets[2] == 21);
    }
    // what apply may not get
    {
        const int64_t offs[3] = {0, 50, 90};
        for (int bad = 0; bad < 9; ++bad) {
            std::vector<Edit> e = {ed(0, 10, 2, "AC"), ed(0, 20, 0, "G"), ed(1, 5, 3, "")};
            if (bad == 0) std::swap(e[0], e[1]);                          // unsorted
            if (bad == 1) e[1].pos = 12;                                  // pos_b - q_a = 0
            if (bad == 2) e[2].pos = 38;                                  // q = 41 > 40
            if (bad == 3) e[2].seq = 2;
            if (bad == 4) e[0].len = 65;
            if (bad == 5) e[0].bases[0] |= 1ull << 4;                     // a bit above 2 * len
            if (bad == 6) e[0].bases[1] = 1;
            if (bad == 7) e[0].pos = -1;
            if (bad == 8) std::swap(e[1], e[2]);                          // sequences out of order
            err.clear();
            CHECK(check_edits(e.data(), e.size(), 2, offs, err) == -1 && !err.empty());
        }
        std::vector<Edit> ok = {ed(0, 0, 0, std::string(64, 'T')), ed(0, 1, 49, ""), ed(1, 40, 0, "A")};      // an insertion at a sequence's end
        CHECK(check_edits(ok.data(), ok.size(), 2, offs, err) == 0);
        CHECK(check_edits(nullptr, 0, 0, offs, err) == 0);
    }
    std::printf("ok\n");
    return 0;
}
