// gaps_host_check.cpp -- jasper_amd/csrc/gaps_host.hpp as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_gaps_host.py).  No HIP, no GPU.
//
//   gaps_host_check FILE
//
// FILE holds numbers separated by blanks: k n_seqs max_trim long_runs, the n_seqs lengths, the number of unreliable runs and for each
// (seq start n_kmers min_count), the number of invalid-window runs and for each (seq start n_kmers).  It prints one line per site that
// gap_build_sites makes of them -- seq a q kind status trim_left trim_right ref_min -- then, after its own checks of gap_check_sites,
// gap_check_records and gap_counts on hand-made lists, the line `ok`.
#include "gaps_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>

using namespace jk;

struct URun { int64_t start; uint64_t n_kmers; uint32_t seq, min_count; };
struct IRun { int64_t start; uint64_t n_kmers; uint32_t seq; };

#define REQUIRE(x)                                                       \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);         \
            return 1;                                                    \
        }                                                                \
    } while (0)

static GapSite site(uint32_t seq, int64_t a, int64_t q) {
    GapSite s{};
    s.seq = seq;
    s.a = a;
    s.q = q;
    s.ref_min = 7;
    s.levels = 99;      // (overwritten)
    return s;
}

static int own_checks() {
    std::string err;
    const int k = 5;
    const int64_t offs[3] = {0, 40, 40};                // a sequence of 40 bytes and an empty one
    // explicit sites
    std::vector<GapSite> s = {site(0, 4, 4), site(0, 10, 20), site(0, 36, 36)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) == 0 && s[0].levels == 0 && s[1].ref_min == 7 && s[2].kind == GAP_KIND_EXPLICIT && s[2].status == GAP_NONE);
    s = {site(0, 3, 10)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("out of bounds") != std::string::npos);
    s = {site(0, 10, 37)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("out of bounds") != std::string::npos);
    s = {site(0, 12, 10)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("a > q") != std::string::npos);
    s = {site(2, 10, 12)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("no sequence") != std::string::npos);
    s = {site(1, 4, 4)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0);  // the empty sequence has no room for flanks
    s = {site(0, 10, 12), site(0, 10, 14)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("order") != std::string::npos);
    s = {site(0, 20, 22), site(0, 10, 14)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) != 0 && err.find("order") != std::string::npos);
    s.clear();
    REQUIRE(gap_check_sites(k, 2, offs, s, err) == 0);
    // records
    s = {site(0, 10, 20), site(0, 30, 31)};
    REQUIRE(gap_check_sites(k, 2, offs, s, err) == 0);
    s[0].status = GAP_DEAD;
    s[0].levels = 7;
    s[0].n_records = 2;
    s[1].status = GAP_SKIPPED;
    std::vector<char> pool = {'A', 'C', 'G', 'T', 'A'};
    std::vector<GapFill> f = {GapFill{10, 0, 0, 10, 0, 3}, GapFill{10, 1, 0, 10, 4, 3}};
    REQUIRE(gap_check_records(s, f, pool, 3, 8, err) == 0);
    std::vector<uint64_t> counts;
    gap_counts(2, s, counts);
    REQUIRE(counts.size() == 2 * GAP_COUNTS && counts[0] == 2 && counts[1] == 1 && counts[2] == 1 && counts[3] == 0 && counts[4] == 2 && counts[9] == 0);
    auto refused = [&](std::vector<GapSite> ss, std::vector<GapFill> ff, std::vector<char> pp) { return gap_check_records(ss, ff, pp, 3, 8, err) != 0; };
    std::vector<GapFill> g = f;
    g[1].bases_off = 2;                                 // past the pool's end
    REQUIRE(refused(s, g, pool));
    g = f;
    g[1].len = 8;                                       // longer than the search went
    REQUIRE(refused(s, g, pool));
    g = f;
    g[0].pos = 11;                                      // of no site
    REQUIRE(refused(s, g, pool));
    g = f;
    g[0].ref_len = 9;
    REQUIRE(refused(s, g, pool));
    g = f;
    g[0].alt_min = 2;                                   // below the threshold
    REQUIRE(refused(s, g, pool));
    g = f;
    g[0].pos = 30;                                      // a record of a skipped site
    g[0].ref_len = 1;
    REQUIRE(refused(s, g, pool));
    std::vector<char> bad = pool;
    bad[2] = 'g';
    REQUIRE(refused(s, f, bad));
    g = f;
    g.pop_back();                                       // fewer than the site says
    REQUIRE(refused(s, g, pool));
    std::vector<GapSite> t = s;
    t[1].status = GAP_NONE;                             // a site the search did not see
    REQUIRE(refused(t, f, pool));
    t = s;
    t[0].status = GAP_LIMIT;                            // limit at another level than max_len
    REQUIRE(refused(t, f, pool));
    t = s;
    t[0].levels = 9;
    REQUIRE(refused(t, f, pool));
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: gaps_host_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int k = 0, n_seqs = 0, long_runs = 0;
    int64_t max_trim = 0;
    in >> k >> n_seqs >> max_trim >> long_runs;
    if (!in || n_seqs < 0) return 2;
    std::vector<int64_t> offs((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; ++i) {
        int64_t len = 0;
        in >> len;
        offs[(size_t)i + 1] = offs[i] + len;
    }
    size_t nu = 0, ni = 0;
    in >> nu;
    std::vector<URun> unrel(nu);
    for (URun &r : unrel) in >> r.seq >> r.start >> r.n_kmers >> r.min_count;
    in >> ni;
    std::vector<IRun> inval(ni);
    for (IRun &r : inval) in >> r.seq >> r.start >> r.n_kmers;
    if (!in) return 2;
    std::vector<GapSite> sites;
    std::string err;
    if (gap_build_sites(k, n_seqs, offs.data(), unrel, inval, max_trim, long_runs != 0, sites, err)) {
        std::printf("error %s\n", err.c_str());
        return 1;
    }
    for (const GapSite &s : sites)
        std::printf("%u %lld %lld %u %u %u %u %u\n", s.seq, (long long)s.a, (long long)s.q, (unsigned)s.kind, (unsigned)s.status, s.trim_left, s.trim_right, s.ref_min);
    if (own_checks()) return 1;
    std::printf("ok\n");
    return 0;
}
