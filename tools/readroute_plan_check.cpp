// readroute_plan_check.cpp -- jasper_amd/csrc/readroute_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -fsanitize=address,undefined -Ijasper_amd/csrc tools/readroute_plan_check.cpp -o readroute_plan_check && ./readroute_plan_check
//
// No HIP, no GPU.  It builds segment lists of every shape the routing meets -- one segment, empty segments, 1 / 15 / 16 / 17 bytes, one
// long record between short ones, sizes across a block and a pass of the block-total scan -- in heap arrays of exactly the size the
// interface states (so that a read past them is caught), checks what route_check accepts and refuses, and what must hold of the buffer
// sizes; `ok` at the end.
#include "readroute_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace jk;

static void need(bool ok, const char *what, uint64_t n, uint64_t n_seg) {
    if (ok) return;
    std::fprintf(stderr, "readroute_plan_check: %s fails at n = %llu, n_seg = %llu\n", what, (unsigned long long)n, (unsigned long long)n_seg);
    std::exit(1);
}

static uint64_t cases = 0;

static void check_sizes(const std::vector<int64_t> &sizes) {
    const uint64_t n_seg = sizes.size();
    std::vector<int64_t> bounds(n_seg + 1);
    std::vector<uint8_t> bins(n_seg);
    bounds[0] = 0;
    for (uint64_t i = 0; i < n_seg; ++i) {
        bounds[i + 1] = bounds[i] + sizes[i];
        bins[i] = (uint8_t)((i * 7 + 1) % RR_BINS);
    }
    const int64_t n = bounds[n_seg];
    need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_OK, "a proper list is accepted", (uint64_t)n, n_seg);
    need(route_check(n + 1, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BOUNDS, "bounds that do not end with n", (uint64_t)n, n_seg);
    if (n_seg) {
        bins[n_seg / 2] = RR_BINS;
        need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BIN, "a bin code of 3", (uint64_t)n, n_seg);
        bins[n_seg / 2] = 255;
        need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BIN, "a bin code of 255", (uint64_t)n, n_seg);
        bins[n_seg / 2] = 0;
        need(route_check(n, (int64_t)n_seg, bounds.data(), nullptr) == RR_BAD_BIN, "no bin codes", (uint64_t)n, n_seg);
        bounds[0] = 1;
        need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BOUNDS, "bounds that do not begin with 0", (uint64_t)n, n_seg);
        bounds[0] = 0;
    }
    if (n_seg >= 2 && sizes[0] > 0) {
        const int64_t keep = bounds[1];
        bounds[1] = -1;
        need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BOUNDS, "a negative bound", (uint64_t)n, n_seg);
        bounds[1] = n + 1;
        need(route_check(n, (int64_t)n_seg, bounds.data(), bins.data()) == RR_BAD_BOUNDS, "a bound beyond n", (uint64_t)n, n_seg);
        bounds[1] = keep;
    }
    need(route_check(n, (int64_t)n_seg, nullptr, bins.data()) == RR_BAD_BOUNDS, "no bounds", (uint64_t)n, n_seg);
    const RouteBuffers b = route_buffers((uint64_t)n, n_seg);
    need(b.text >= (uint64_t)n + 15 + 16 && b.out >= (uint64_t)n + 16, "room around the text and behind the output", (uint64_t)n, n_seg);
    need(b.bounds == (n_seg + 1) * 8 && b.bins >= n_seg && b.bins >= 1, "segment arrays", (uint64_t)n, n_seg);
    need(b.cols >= RR_BINS * n_seg * 8 && b.cols >= RR_BINS * 8 && b.pre == RR_BINS * (n_seg + 1) * 8, "columns and scans", (uint64_t)n, n_seg);
    // the scan's last kernel runs over n_seg + 1 entries: the block that holds the total has a base among the block totals
    need(rt_blocks(n_seg + 1) <= rt_blocks(n_seg) + 1 && b.blocks == RR_BINS * (rt_blocks(n_seg) + 1) * 8, "scan blocks", (uint64_t)n, n_seg);
    need(route_col_words(n_seg) * RR_BINS * 8 == b.cols && route_pre_words(n_seg) * RR_BINS * 8 == b.pre && route_block_words(n_seg) * RR_BINS * 8 == b.blocks,
         "the strides are the sizes", (uint64_t)n, n_seg);
    ++cases;
}

int main() {
    check_sizes({});
    for (int64_t one : {0, 1, 15, 16, 17, RT_BLOCK - 1, RT_BLOCK, RT_BLOCK + 1, 100000}) check_sizes({one});
    check_sizes({0, 0, 0});
    check_sizes({1, 15, 16, 17, 0, 0, 1});
    check_sizes({300, 100000, 300, 0, 300});
    for (uint64_t n_seg : {(uint64_t)RT_BLOCK - 1, (uint64_t)RT_BLOCK, (uint64_t)RT_BLOCK + 1, (uint64_t)RT_BLOCK * RT_SCAN_PASS - 1, (uint64_t)RT_BLOCK * RT_SCAN_PASS,
                           (uint64_t)RT_BLOCK * RT_SCAN_PASS + 1}) {
        std::vector<int64_t> sizes(n_seg);
        for (uint64_t i = 0; i < n_seg; ++i) sizes[i] = (int64_t)(i % 5);
        check_sizes(sizes);
    }
    // the limits: refused by their size alone, before an array is looked at
    const int64_t zero = 0;
    need(route_check(RT_MAX_TEXT + 1, 1, &zero, nullptr) == RR_TOO_LARGE, "a text of 2^31 bytes", (uint64_t)RT_MAX_TEXT + 1, 1);
    need(route_check(-1, 1, &zero, nullptr) == RR_TOO_LARGE, "a negative length", 0, 1);
    need(route_check(0, RR_MAX_SEGMENTS + 1, &zero, nullptr) == RR_TOO_LARGE, "2^31 segments", 0, (uint64_t)RR_MAX_SEGMENTS + 1);
    need(route_check(0, -1, &zero, nullptr) == RR_TOO_LARGE, "a negative segment count", 0, 0);
    const RouteBuffers big = route_buffers((uint64_t)RT_MAX_TEXT, (uint64_t)RR_MAX_SEGMENTS);
    need(big.text > (uint64_t)RT_MAX_TEXT && big.pre == RR_BINS * ((uint64_t)RR_MAX_SEGMENTS + 1) * 8, "the largest call's sizes do not wrap", (uint64_t)RT_MAX_TEXT,
         (uint64_t)RR_MAX_SEGMENTS);
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
