// dups_host_check.cpp -- the host side of the duplication map (jasper_amd/csrc/dups_host.hpp: the encoding, the sequence of a global
// position, the device's runs made public) as a stand-alone program, for a sanitizer build on a machine without a GPU:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I jasper_amd/csrc tools/dups_host_check.cpp -o /tmp/dp_check && /tmp/dp_check
// Prints `ok` and exits 0, or says what differs and exits 1.  (The stitching of partial runs is the shared device stitcher's: no host
// code of it to check here.)
#include "dups_host.hpp"
#include <cstdio>
#include <random>

using namespace jk;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// a run as the device leaves it: the mate of its first window as a global position, nothing in mate_seq
static DupRun dev(uint32_t seq, int64_t start, uint64_t n, int64_t mate_global, uint32_t strand) {
    DupRun r{};
    r.seq = seq;
    r.start = start;
    r.n_kmers = n;
    r.mate_start = mate_global;
    r.strand = strand;
    r.mate_seq = 0xFFFFFFFFu;
    r.pad = 7;
    return r;
}

int main() {
    std::string err;
    CHECK(dup_encode(0, 0) == 0 && dup_encode(0, 1) == 1 && dup_encode(5, 0) == 10 && dup_encode(5, 3) == 11);
    CHECK(dup_encode(5000000000ll, 1) == 10000000001ull);
    // the sequence of a position: boundaries, empty sequences before and between
    {
        const int64_t offs[7] = {0, 0, 100, 100, 100, 250, 5000000250ll};      // sequences 0, 2 and 3 are empty
        CHECK(dup_seq_of(0, 6, offs) == 1 && dup_seq_of(99, 6, offs) == 1);
        CHECK(dup_seq_of(100, 6, offs) == 4 && dup_seq_of(249, 6, offs) == 4);
        CHECK(dup_seq_of(250, 6, offs) == 5 && dup_seq_of(5000000249ll, 6, offs) == 5);
    }
    const int k = 5;
    const int64_t offs[4] = {0, 100, 130, 400};         // windows: 96, 26, 266
    // `+`: the mate of the first window is the leftmost; at a sequence's first and last window
    {
        std::vector<DupRun> r = {dev(0, 10, 20, 100, 0), dev(0, 40, 6, 120, 0), dev(2, 0, 96, 0, 0), dev(1, 3, 1, 395, 0)};
        CHECK(dup_finish_runs(r, k, 3, offs, err) == 0);
        CHECK(r[0].mate_seq == 1 && r[0].mate_start == 0 && r[0].pad == 0 && r[0].start == 10 && r[0].n_kmers == 20);
        CHECK(r[1].mate_seq == 1 && r[1].mate_start == 20);      // windows 20 .. 25: the last six of sequence 1
        CHECK(r[2].mate_seq == 0 && r[2].mate_start == 0);       // every window of sequence 0
        CHECK(r[3].mate_seq == 2 && r[3].mate_start == 265);     // the last window of sequence 2
    }
    // `-`: the mates descend, the leftmost is the mate of the run's last window
    {
        std::vector<DupRun> r = {dev(0, 10, 20, 119, 1), dev(2, 7, 26, 125, 1), dev(0, 0, 1, 130, 1), dev(1, 0, 5, 4, 1)};
        CHECK(dup_finish_runs(r, k, 3, offs, err) == 0);
        CHECK(r[0].mate_seq == 1 && r[0].mate_start == 0 && r[0].strand == 1);
        CHECK(r[1].mate_seq == 1 && r[1].mate_start == 0);       // 125 - 25 = 100: all of sequence 1
        CHECK(r[2].mate_seq == 2 && r[2].mate_start == 0);
        CHECK(r[3].mate_seq == 0 && r[3].mate_start == 0);
    }
    // what cannot be: a stretch that leaves its sequence's windows, on either side, or the text
    {
        for (int bad = 0; bad < 5; ++bad) {
            std::vector<DupRun> r = {bad == 0   ? dev(0, 0, 7, 120, 0)      // windows 20 .. 26 of sequence 1, which has 26
                                     : bad == 1 ? dev(0, 0, 3, 97, 0)       // 97 .. 99 are no window starts of sequence 0 (k = 5)
                                     : bad == 2 ? dev(0, 0, 4, 102, 1)      // descends to 99: across the boundary
                                     : bad == 3 ? dev(0, 0, 2, 0, 1)        // descends below 0
                                                : dev(0, 0, 1, 400, 0)};    // past the text
            err.clear();
            CHECK(dup_finish_runs(r, k, 3, offs, err) == -1 && !err.empty());
        }
        std::vector<DupRun> none;
        CHECK(dup_finish_runs(none, k, 0, offs, err) == 0);
    }
    // many: a run made from a public form comes back as that form
    {
        std::mt19937_64 rng(3);
        const int64_t big[5] = {0, 3000000000ll, 3000000000ll, 7000000000ll, 7000000040ll};
        for (int it = 0; it < 2000; ++it) {
            const int s = (int)(rng() % 4) == 1 ? 0 : (int)(rng() % 4);
            if (big[s + 1] - big[s] < k) continue;
            const int64_t nw = big[s + 1] - big[s] - k + 1;
            const uint64_t n = 1 + rng() % (uint64_t)std::min<int64_t>(nw, 1000);
            const int64_t left = (int64_t)(rng() % (uint64_t)(nw - (int64_t)n + 1));
            const uint32_t strand = (uint32_t)(rng() & 1);
            std::vector<DupRun> r = {dev(0, 0, n, big[s] + (strand ? left + (int64_t)n - 1 : left), strand)};
            CHECK(dup_finish_runs(r, k, 4, big, err) == 0);
            CHECK((int)r[0].mate_seq == s && r[0].mate_start == left);
        }
    }
    std::printf("ok\n");
    return 0;
}
