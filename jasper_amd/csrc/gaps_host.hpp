// gaps_host.hpp -- the host side of the gap scan (gaps.hip): the site and the fill record, the sites made from the two run lists, the
// check of a caller's own site list, the check of what the search hands back, and the per-sequence counters.  Plain C++, nothing of
// HIP, so that tools/gaps_host_check.cpp can build it alone (semantics: include/jasper_hip.h, jasper_gap_scan).
//
// A window is NOT SOLID when it is invalid (it holds a non-base byte: gap_runs_kernel lists those) or unreliable (the report lists
// those).  The two kinds never overlap, so a STRETCH -- a maximal run of windows that are not solid -- is a maximal chain of runs of the
// two lists in which each run starts where the one before it ends.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace jk {

constexpr int GAP_FRONT = 64;            // the search keeps at most this many strings of one length
constexpr int GAP_MAX_RECORDS = 16;      // ... and lists at most this many fills of one site
constexpr int GAP_MAX_LEN = 4096;        // the longest fill that is searched
constexpr int GAP_RUN_MIN = 64;          // a stretch without a non-base byte is a site when it replaces more bytes than this (the compound scan's `long`)

enum { GAP_KIND_EXPLICIT = 0, GAP_KIND_GAP = 1, GAP_KIND_RUN = 2 };
enum { GAP_NONE = 0, GAP_DEAD = 1, GAP_LIMIT = 2, GAP_COMPLEX = 3, GAP_EDGE = 4, GAP_RAGGED = 5, GAP_SKIPPED = 6 };

// where a search starts and ends, and how it ended (layout of the public jasper_gap_site)
struct GapSite {
    int64_t a, q;                  // the R = q - a bytes s[a .. q) are what a fill replaces
    uint32_t seq;
    uint32_t ref_min;
    uint32_t n_records;
    uint32_t levels;               // the t at which the search ended
    uint32_t trim_left, trim_right;
    uint8_t kind, status;
    uint8_t pad[6];
};
static_assert(sizeof(GapSite) == 48, "layout of jasper_gap_site");

// a fill the reads hold (layout of the public jasper_gap_fill); its y is len upper-case letters at bases_off of the result's byte pool
struct GapFill {
    int64_t pos;                   // a
    uint64_t bases_off;
    uint32_t seq;
    uint32_t ref_len;              // R
    uint32_t len;
    uint32_t alt_min;
};
static_assert(sizeof(GapFill) == 32, "layout of jasper_gap_fill");

constexpr int GAP_COUNTS = 9;            // per sequence: sites, searched, bridged, unique, records, edge, ragged, limit, complex

inline bool gap_site_before(const GapSite &x, const GapSite &y) { return x.seq != y.seq ? x.seq < y.seq : x.a < y.a; }

// The sites of n_seqs sequences from the unreliable runs (start, n_kmers, seq, min_count) and the invalid-window runs (start, n_kmers,
// seq), both in (seq, start) order; offsets are the n_seqs + 1 boundaries of the text.  -1 and a message when the lists are not what
// the two scans of that text can have written.
template <class URun, class IRun>
inline int gap_build_sites(int k, int n_seqs, const int64_t *offsets, const std::vector<URun> &unrel, const std::vector<IRun> &inval, int64_t max_trim, bool long_runs,
                           std::vector<GapSite> &sites, std::string &err) {
    sites.clear();
    size_t iu = 0, ii = 0;
    int64_t end_before = -1;
    uint32_t seq_before = 0;
    while (iu < unrel.size() || ii < inval.size()) {
        // the next run of either list opens a stretch ...
        bool from_u = ii >= inval.size() || (iu < unrel.size() && (unrel[iu].seq != inval[ii].seq ? unrel[iu].seq < inval[ii].seq : unrel[iu].start < inval[ii].start));
        const uint32_t seq = from_u ? unrel[iu].seq : inval[ii].seq;
        if (seq >= (uint32_t)n_seqs) { err = "gap scan: a run of no sequence"; return -1; }
        const int64_t n = offsets[seq + 1] - offsets[seq];
        const int64_t u0 = from_u ? unrel[iu].start : inval[ii].start;
        if (u0 < 0 || (end_before >= 0 && (seq < seq_before || (seq == seq_before && u0 <= end_before)))) { err = "gap scan: the runs overlap or are out of order"; return -1; }
        int64_t next = u0, first_inv = -1, last_inv = -1;
        uint32_t ref_min = 0xFFFFFFFFu;
        bool any_valid = false;
        // ... and every run that starts where the stretch ends so far continues it
        for (;;) {
            if (iu < unrel.size() && unrel[iu].seq == seq && unrel[iu].start == next) {
                if (unrel[iu].n_kmers == 0) { err = "gap scan: an empty run"; return -1; }
                ref_min = std::min<uint32_t>(ref_min, unrel[iu].min_count);
                any_valid = true;
                next += (int64_t)unrel[iu].n_kmers;
                ++iu;
            } else if (ii < inval.size() && inval[ii].seq == seq && inval[ii].start == next) {
                if (inval[ii].n_kmers == 0) { err = "gap scan: an empty run"; return -1; }
                if (first_inv < 0) first_inv = next;
                next += (int64_t)inval[ii].n_kmers;
                last_inv = next - 1;
                ++ii;
            } else {
                break;
            }
        }
        const int64_t u1 = next - 1;
        if (u1 > n - k) { err = "gap scan: a run past its sequence's last window"; return -1; }
        end_before = u1;
        seq_before = seq;
        GapSite S{};
        S.kind = first_inv >= 0 ? GAP_KIND_GAP : GAP_KIND_RUN;
        if (S.kind == GAP_KIND_RUN && (!long_runs || u1 - u0 + 2 - k <= GAP_RUN_MIN)) continue;      // not a site
        S.a = u0 + k - 1;
        S.q = u1 + 1;
        S.seq = seq;
        S.ref_min = any_valid ? ref_min : 0u;
        if (u0 == 0 || u1 == n - k) {
            S.status = GAP_EDGE;                            // no solid window on that side (the trims stay 0)
        } else {
            if (S.kind == GAP_KIND_GAP) {
                S.trim_left = (uint32_t)std::min<int64_t>(first_inv - u0, 0xFFFFFFFFll);      // = (first non-base byte) - a
                S.trim_right = (uint32_t)std::min<int64_t>(u1 - last_inv, 0xFFFFFFFFll);      // = q - (last non-base byte + 1)
            }
            if ((int64_t)S.trim_left > max_trim || (int64_t)S.trim_right > max_trim) S.status = GAP_RAGGED;
        }
        sites.push_back(S);
    }
    return 0;
}

// A caller's own sites: in (seq, a) order, no two at one place, k - 1 <= a <= q <= n - (k - 1).  Everything but seq, a, q and ref_min is
// set to what an unsearched explicit site holds.
inline int gap_check_sites(int k, int n_seqs, const int64_t *offsets, std::vector<GapSite> &sites, std::string &err) {
    for (size_t i = 0; i < sites.size(); ++i) {
        GapSite &S = sites[i];
        if (S.seq >= (uint32_t)n_seqs) { err = "gap search: a site of no sequence"; return -1; }
        const int64_t n = offsets[S.seq + 1] - offsets[S.seq];
        if (S.a > S.q) { err = "gap search: a site with a > q"; return -1; }
        if (S.a < k - 1 || S.q > n - (k - 1)) { err = "gap search: a site whose flanks are out of bounds (k - 1 <= a <= q <= n - (k - 1))"; return -1; }
        if (i && !gap_site_before(sites[i - 1], S)) { err = "gap search: the sites are not in (seq, a) order"; return -1; }
        const GapSite in = S;
        S = GapSite{};
        S.a = in.a;
        S.q = in.q;
        S.seq = in.seq;
        S.ref_min = in.ref_min;
        S.kind = GAP_KIND_EXPLICIT;
    }
    return 0;
}

// What the search handed back: a record it cannot have written, or a site it cannot have left so, is refused.  sites are in (seq, a) order.
inline int gap_check_records(const std::vector<GapSite> &sites, const std::vector<GapFill> &fills, const std::vector<char> &pool, uint32_t thre, int max_len, std::string &err) {
    std::vector<uint32_t> seen(sites.size(), 0);
    for (const GapFill &v : fills) {
        GapSite key{};
        key.seq = v.seq;
        key.a = v.pos;
        const auto s = std::lower_bound(sites.begin(), sites.end(), key, gap_site_before);
        bool ok = s != sites.end() && s->seq == v.seq && s->a == v.pos && (int64_t)v.ref_len == s->q - s->a && (int64_t)v.len <= (int64_t)max_len && v.len <= s->levels &&
                  s->status >= GAP_DEAD && s->status <= GAP_COMPLEX && v.alt_min >= thre && v.bases_off <= pool.size() && v.len <= pool.size() - v.bases_off;
        for (uint32_t i = 0; ok && i < v.len; ++i) {
            const char c = pool[v.bases_off + i];
            ok = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        }
        if (!ok) { err = "gap scan: a record the search cannot have written"; return -1; }
        ++seen[(size_t)(s - sites.begin())];
    }
    for (size_t i = 0; i < sites.size(); ++i) {
        const GapSite &S = sites[i];
        const bool searched = S.status >= GAP_DEAD && S.status <= GAP_COMPLEX;
        if (S.status == GAP_NONE || S.status > GAP_SKIPPED || seen[i] != S.n_records || S.n_records > (uint32_t)GAP_MAX_RECORDS || (!searched && (S.n_records || S.levels)) ||
            (int64_t)S.levels > (int64_t)max_len ||(S.status == GAP_LIMIT && (int64_t)S.levels != max_len)) {
            err = "gap scan: a site the search cannot have left so";
            return -1;
        }
    }
    return 0;
}

// the nine counters per sequence
inline void gap_counts(int n_seqs, const std::vector<GapSite> &sites, std::vector<uint64_t> &counts) {
    counts.assign((size_t)n_seqs * GAP_COUNTS, 0);
    for (const GapSite &S : sites) {
        uint64_t *c = &counts[(size_t)S.seq * GAP_COUNTS];
        ++c[0];
        if (S.status >= GAP_DEAD && S.status <= GAP_COMPLEX) ++c[1];
        if (S.n_records) ++c[2];
        if (S.n_records == 1 && S.status != GAP_COMPLEX) ++c[3];
        c[4] += S.n_records;
        if (S.status == GAP_EDGE) ++c[5];
        if (S.status == GAP_RAGGED) ++c[6];
        if (S.status == GAP_LIMIT) ++c[7];
        if (S.status == GAP_COMPLEX) ++c[8];
    }
}

}  // namespace jk
