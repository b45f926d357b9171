// hetcluster_host_check.cpp -- the host side of the het-cluster search (jasper_amd/csrc/hetcluster_host.hpp: refuse, sort, count) as a
// stand-alone program, for a sanitizer build on a machine without a GPU:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I jasper_amd/csrc tools/hetcluster_host_check.cpp -o /tmp/hc_check && /tmp/hc_check
// Prints `ok` and exits 0, or says what differs and exits 1.
#include "hetcluster_host.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace jk;

static HetCluster rec(uint32_t seq, int64_t pos, uint32_t rlen, const std::string &y) {
    HetCluster v;
    std::memset(&v, 0, sizeof v);
    v.seq = seq;
    v.pos = pos;
    v.ref_len = rlen;
    v.len = (uint16_t)y.size();
    v.ref_min = 5;
    v.alt_min = 4;
    for (size_t i = 0; i < y.size(); ++i) v.bases[i >> 5] |= (uint64_t)(std::strchr("ACGT", y[i]) - "ACGT") << (2 * (i & 31));
    return v;
}
static std::string str(const HetCluster &v) {
    std::string y;
    for (int i = 0; i < (int)v.len; ++i) y += "ACGT"[het_cluster_base(v, i)];
    return y;
}
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main() {
    std::string err;
    const std::string y64(64, 'T');
    // sites are candidates (pos, first base); the order is (seq, pos, ref_len, len, y)
    std::vector<HetCluster> recs = {rec(1, 9, 2, "GA"),   rec(0, 7, 3, "CAT"), rec(0, 7, 2, "GT"), rec(0, 7, 3, "CAG"), rec(0, 7, 3, "CA"),
                                    rec(0, 7, 64, y64),   rec(2, 0, 1, "AC"),  rec(0, 3, 5, "ACGTA"), rec(0, 7, 2, "CT")};
    std::vector<uint64_t> counts(4 * 3, 0);
    counts[0] = 11;                                                   // searched and complex are the kernel's: left alone
    counts[3] = 2;
    CHECK(het_cluster_finish(recs, 3, 64, counts, err) == 0);
    const char *want[] = {"ACGTA", "CT", "GT", "CA", "CAG", "CAT", y64.c_str(), "GA", "AC"};
    for (size_t i = 0; i < recs.size(); ++i) CHECK(str(recs[i]) == want[i]);
    const uint64_t wc[12] = {11, 4, 7, 2, 0, 1, 1, 0, 0, 1, 1, 0};   // seq 0: (3, A), (7, C), (7, G), (7, T)
    for (int i = 0; i < 12; ++i) CHECK(counts[i] == wc[i]);
    // what the kernel cannot have written
    for (int bad = 0; bad < 8; ++bad) {
        std::vector<HetCluster> one = {rec(0, 7, 3, "CAT")};
        std::vector<uint64_t> c4(4, 0);
        if (bad == 0) one[0].seq = 1;
        if (bad == 1) one[0].ref_len = 0;
        if (bad == 2) one[0].ref_len = 5;
        if (bad == 3) one[0].len = 0;
        if (bad == 4) one[0].len = 5;
        if (bad == 5) one[0].bases[0] |= 1ull << 6;                   // a bit above 2 * len
        if (bad == 6) one[0].bases[1] = 1;
        if (bad == 7) one[0].pos = -1;
        err.clear();
        CHECK(het_cluster_finish(one, 1, 4, c4, err) == -1 && !err.empty() && c4[1] == 0 && c4[2] == 0);
    }
    {
        std::vector<HetCluster> one = {rec(0, 7, 40, std::string(40, 'G'))};
        std::vector<uint64_t> c4(4, 0);
        one[0].bases[1] |= 1ull << 16;                                // base 40 of a record of 40
        CHECK(het_cluster_finish(one, 1, 64, c4, err) == -1);
    }
    // nothing, and many: sorted, counted, every record kept
    std::vector<HetCluster> none;
    std::vector<uint64_t> c0;
    CHECK(het_cluster_finish(none, 0, 64, c0, err) == 0);
    std::mt19937_64 rng(7);
    std::vector<HetCluster> many;
    for (int i = 0; i < 20000; ++i) {
        std::string y(1 + rng() % 64, 'A');
        for (char &ch : y) ch = "ACGT"[rng() % 4];
        many.push_back(rec((uint32_t)(rng() % 5), (int64_t)(rng() % 50), 1 + (uint32_t)(rng() % 64), y));
    }
    std::vector<uint64_t> c5(4 * 5, 0);
    CHECK(het_cluster_finish(many, 5, 64, c5, err) == 0 && many.size() == 20000);
    uint64_t nrec = 0;
    for (int s = 0; s < 5; ++s) {
        nrec += c5[4 * s + 2];
        CHECK(c5[4 * s + 1] <= 200 && c5[4 * s + 1] <= c5[4 * s + 2]);
    }
    CHECK(nrec == 20000);
    for (size_t i = 1; i < many.size(); ++i) {
        const HetCluster &a = many[i - 1], &b = many[i];
        CHECK(a.seq <= b.seq && (a.seq < b.seq || a.pos <= b.pos) && (a.seq < b.seq || a.pos < b.pos || a.ref_len <= b.ref_len));
        if (a.seq == b.seq && a.pos == b.pos && a.ref_len == b.ref_len) CHECK(a.len < b.len || (a.len == b.len && str(a) <= str(b)));
    }
    std::printf("ok\n");
    return 0;
}
