// repair_host.hpp -- the host side of the repair stage (repair.hip): the edit record, the scans' error records made edits, the selection
// of the edits one round applies, the plan of where they land in the new text, and the check of an edit list a caller hands in
// (semantics: include/jasper_hip.h, jasper_repair).  Plain C++ with no HIP in it, so that it also compiles into a stand-alone program
// (tools/repair_host_check.cpp).  The scans' record types are template arguments: only their field names are used.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace jk {

constexpr int REPAIR_MAX_Y = 64, REPAIR_MAX_ROUNDS = 8;
enum { ES_SUB = 1, ES_INS = 2, ES_DEL = 3, ES_MIXED = 4, ES_COMPOUND = 5 };      // where an edit comes from
constexpr uint8_t EDIT_KIND_ERROR = 2;                                           // VK_ERROR (variants.hpp)

// "the reads hold y where the sequence holds the ref_len bytes from pos on" (layout of the public jasper_edit: that of jasper_compound
// with source and round in two of its pad bytes)
struct Edit {
    int64_t pos;
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint32_t ref_len;              // R
    uint64_t bases[2];             // base i of y in bits 2i, 2i + 1 (of bases[i / 32]); 0 above 2 * len
    uint16_t len;                  // |y|
    uint8_t source;                // ES_*
    uint8_t round;                 // 1 ..: the round that applied it (0 in a caller's list)
    uint8_t pad[4];
};
static_assert(sizeof(Edit) == 48, "layout of jasper_edit");
static_assert(offsetof(Edit, pos) == 0 && offsetof(Edit, seq) == 8 && offsetof(Edit, ref_min) == 12 && offsetof(Edit, alt_min) == 16 && offsetof(Edit, ref_len) == 20 &&
                  offsetof(Edit, bases) == 24 && offsetof(Edit, len) == 40 && offsetof(Edit, source) == 42 && offsetof(Edit, round) == 43,
              "layout of jasper_edit");

inline unsigned edit_base(const Edit &e, int i) { return (unsigned)(e.bases[i >> 5] >> (2 * (i & 31))) & 3u; }
inline void edit_push(Edit &e, unsigned code) {
    e.bases[e.len >> 5] |= (uint64_t)(code & 3u) << (2 * (e.len & 31));
    ++e.len;
}
inline int64_t edit_end(const Edit &e) { return e.pos + (int64_t)e.ref_len; }      // q
// y of a against y of b as strings: < 0, 0, > 0
inline int edit_cmp_y(const Edit &a, const Edit &b) {
    const int n = std::min<int>(a.len, b.len);
    for (int i = 0; i < n; ++i)
        if (edit_base(a, i) != edit_base(b, i)) return edit_base(a, i) < edit_base(b, i) ? -1 : 1;
    return (int)a.len - (int)b.len;
}
inline Edit edit_make(uint32_t seq, int64_t pos, uint32_t ref_len, uint32_t ref_min, uint32_t alt_min, int source) {
    Edit e{};
    e.pos = pos;
    e.seq = seq;
    e.ref_min = ref_min;
    e.alt_min = alt_min;
    e.ref_len = ref_len;
    e.source = (uint8_t)source;
    return e;
}
inline int edit_letter_code(uint8_t ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1; }

// ---- normalisation: records of kind error -> edits (het records are never applied) -------------------------------------------------
template <class V> int edits_from_variants(const std::vector<V> &recs, std::vector<Edit> &out, std::string &err) {
    for (const V &v : recs) {
        if (v.kind != EDIT_KIND_ERROR) continue;
        const int c = edit_letter_code(v.alt);
        if (c < 0) { err = "repair: a substitution whose alternative is no base"; return -1; }
        Edit e = edit_make(v.seq, v.pos, 1, v.ref_min, v.alt_min, ES_SUB);
        edit_push(e, (unsigned)c);
        out.push_back(e);
    }
    return 0;
}
template <class I> int edits_from_indels(const std::vector<I> &recs, std::vector<Edit> &out, std::string &err) {
    for (const I &v : recs) {
        if (v.kind != EDIT_KIND_ERROR) continue;
        if (v.type == 2) {                              // IT_DEL: the len bytes from pos on go
            out.push_back(edit_make(v.seq, v.pos, v.len, v.ref_min, v.alt_min, ES_DEL));
            continue;
        }
        const int c = edit_letter_code(v.base);
        if (v.type != 1 || c < 0 || v.len < 1 || v.len > REPAIR_MAX_Y) { err = "repair: an insertion the indel scan cannot have written"; return -1; }
        Edit e = edit_make(v.seq, v.pos, 0, v.ref_min, v.alt_min, ES_INS);
        for (int i = 0; i < (int)v.len; ++i) edit_push(e, (unsigned)c);
        out.push_back(e);
    }
    return 0;
}
template <class M> int edits_from_mixed(const std::vector<M> &recs, std::vector<Edit> &out, std::string &err) {
    for (const M &v : recs) {
        if (v.kind != EDIT_KIND_ERROR) continue;
        if (v.len < 1 || v.len > 16) { err = "repair: a mixed insertion the indel scan cannot have written"; return -1; }
        Edit e = edit_make(v.seq, v.pos, 0, v.ref_min, v.alt_min, ES_MIXED);
        for (int i = 0; i < (int)v.len; ++i) edit_push(e, (v.bases >> (2 * i)) & 3u);
        out.push_back(e);
    }
    return 0;
}
template <class Cp> int edits_from_compound(const std::vector<Cp> &recs, std::vector<Edit> &out, std::string &err) {
    for (const Cp &v : recs) {                          // every compound record is an error
        if (v.len < 1 || v.len > REPAIR_MAX_Y || v.ref_len < 1) { err = "repair: a compound record the search cannot have written"; return -1; }
        Edit e = edit_make(v.seq, v.pos, v.ref_len, v.ref_min, v.alt_min, ES_COMPOUND);
        e.bases[0] = v.bases[0];
        e.bases[1] = v.bases[1];
        e.len = v.len;
        out.push_back(e);
    }
    return 0;
}

// ---- selection -------------------------------------------------------------------------------------------------------------------------
struct Selection {
    std::vector<Edit> accepted;     // ordered by (seq, pos)
    uint64_t records = 0;           // edits after the duplicates were dropped: accepted + conflicts + ambiguous
    uint64_t conflicts = 0, ambiguous = 0;
};

// One round's choice among `edits` (any order; it is reordered).  Edits with one (seq, pos, ref_len, y) are one edit: the first source
// stays.  Edits that share (seq, pos, ref_len, |y|, alt_min) and differ in y are ambiguous and all set aside.  The rest is gone through
// by (ref_len + |y| ascending, alt_min descending, seq, pos, ref_len, y): an edit is accepted unless it conflicts with an accepted one --
// two edits a, b of one sequence with (pos_a, q_a) <= (pos_b, q_b) conflict iff pos_b - q_a < k - 1.
inline void select_edits(std::vector<Edit> &edits, int k, Selection &S) {
    S = Selection();
    std::stable_sort(edits.begin(), edits.end(), [](const Edit &a, const Edit &b) {
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len;
        if (a.len != b.len) return a.len < b.len;
        const int c = edit_cmp_y(a, b);
        if (c) return c < 0;
        return a.source < b.source;
    });
    auto same_site = [](const Edit &a, const Edit &b) { return a.seq == b.seq && a.pos == b.pos && a.ref_len == b.ref_len && a.len == b.len; };
    edits.erase(std::unique(edits.begin(), edits.end(), [&](const Edit &a, const Edit &b) { return same_site(a, b) && edit_cmp_y(a, b) == 0; }), edits.end());
    S.records = edits.size();
    std::vector<Edit> rest;
    for (size_t i = 0; i < edits.size();) {             // (one site and length: contiguous, in y order)
        size_t j = i + 1;
        while (j < edits.size() && same_site(edits[i], edits[j])) ++j;
        for (size_t a = i; a < j; ++a) {
            bool tie = false;
            for (size_t b = i; b < j && !tie; ++b) tie = b != a && edits[b].alt_min == edits[a].alt_min;
            if (tie) ++S.ambiguous;
            else rest.push_back(edits[a]);
        }
        i = j;
    }
    std::sort(rest.begin(), rest.end(), [](const Edit &a, const Edit &b) {
        const uint32_t wa = a.ref_len + a.len, wb = b.ref_len + b.len;
        if (wa != wb) return wa < wb;
        if (a.alt_min != b.alt_min) return a.alt_min > b.alt_min;
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len;
        return edit_cmp_y(a, b) < 0;
    });
    // the accepted edits of one sequence lie at least k - 1 >= 1 bytes apart, so in (pos, q) order their q ascend too: only the two
    // neighbours of a new edit in that order can conflict with it
    typedef std::tuple<uint32_t, int64_t, int64_t> Key;      // (seq, pos, q)
    std::set<Key> taken;
    const int64_t gap = (int64_t)k - 1;
    for (const Edit &e : rest) {
        const Key key(e.seq, e.pos, edit_end(e));
        auto nx = taken.lower_bound(key);
        bool clash = false;
        if (nx != taken.end() && std::get<0>(*nx) == e.seq) clash = *nx == key || std::get<1>(*nx) - edit_end(e) < gap;
        if (!clash && nx != taken.begin()) {
            auto pv = std::prev(nx);
            if (std::get<0>(*pv) == e.seq) clash = e.pos - std::get<2>(*pv) < gap;
        }
        if (clash) { ++S.conflicts; continue; }
        taken.insert(key);
        S.accepted.push_back(e);
    }
    std::sort(S.accepted.begin(), S.accepted.end(), [](const Edit &a, const Edit &b) { return a.seq != b.seq ? a.seq < b.seq : a.pos < b.pos; });
}

// ---- the list apply gets -----------------------------------------------------------------------------------------------------------------
// Refuses what apply may not get: a sequence out of range, |y| > 64, bits above 2 * |y|, q beyond the sequence, a list that is not in
// (seq, pos) order, two edits of one sequence with pos_b - q_a < 1.  offsets: n_seqs + 1 entries.
inline int check_edits(const Edit *edits, uint64_t n, int n_seqs, const int64_t *offsets, std::string &err) {
    for (uint64_t i = 0; i < n; ++i) {
        const Edit &e = edits[i];
        if (e.seq >= (uint32_t)(n_seqs < 0 ? 0 : n_seqs)) { err = "apply edits: an edit of no sequence"; return -1; }
        if (e.len > REPAIR_MAX_Y) { err = "apply edits: a replacement of more than 64 bases"; return -1; }
        bool clean = true;
        if (e.len < 32) clean = (e.bases[0] >> (2 * e.len)) == 0 && e.bases[1] == 0;
        else if (e.len < 64) clean = (e.bases[1] >> (2 * (e.len - 32))) == 0;
        if (!clean) { err = "apply edits: bits above the replacement's last base"; return -1; }
        const int64_t len = offsets[e.seq + 1] - offsets[e.seq];
        if (e.pos < 0 || e.pos > len || (int64_t)e.ref_len > len - e.pos) { err = "apply edits: an edit that ends beyond its sequence"; return -1; }
        if (i) {
            const Edit &p = edits[i - 1];
            if (p.seq > e.seq || (p.seq == e.seq && p.pos > e.pos)) { err = "apply edits: the edits are not in (sequence, position) order"; return -1; }
            if (p.seq == e.seq && e.pos - edit_end(p) < 1) { err = "apply edits: two edits less than one byte apart"; return -1; }
        }
    }
    return 0;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------
// Where a checked edit list lands: src[i] / dst[i] = the first byte edit i replaces in the old text and the first byte of its y in the new
// one, both counted from the start of the whole text; new_offsets = the sequences' boundaries afterwards.
struct EditPlan {
    std::vector<int64_t> src, dst, new_offsets;
};
inline void plan_edits(const Edit *edits, uint64_t n, int n_seqs, const int64_t *offsets, EditPlan &P) {
    P.src.resize(n);
    P.dst.resize(n);
    P.new_offsets.assign((size_t)n_seqs + 1, 0);
    int64_t delta = 0;                                  // new minus old position of the bytes after the edits so far
    uint64_t i = 0;
    for (int s = 0; s < n_seqs; ++s) {
        P.new_offsets[s] = offsets[s] - offsets[0] + delta;
        for (; i < n && edits[i].seq == (uint32_t)s; ++i) {
            P.src[i] = offsets[s] - offsets[0] + edits[i].pos;
            P.dst[i] = P.src[i] + delta;
            delta += (int64_t)edits[i].len - (int64_t)edits[i].ref_len;
        }
    }
    P.new_offsets[n_seqs] = offsets[n_seqs] - offsets[0] + delta;
}

}  // namespace jk
