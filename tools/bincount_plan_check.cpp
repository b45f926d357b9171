// bincount_plan_check.cpp -- jasper_amd/csrc/bincount_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -fsanitize=address,undefined -Ijasper_amd/csrc tools/bincount_plan_check.cpp -o bincount_plan_check && ./bincount_plan_check
//
// No HIP, no GPU.  It builds batches of every shape the gather meets -- no read, empty reads, 1 / 15 / 16 / 17 bytes, one long read
// between short ones, runs of reads no sink takes -- in heap arrays of exactly the size the interface states (so that a read past them is
// caught), and for every mask and a row of piece sizes checks what bincount_check accepts and refuses, a sink's list against a plain
// restatement, and what must hold of the pieces: whole reads, in order, every read once, no piece above the piece size unless it is one
// read, no piece above the room its buffer has; `ok` at the end.
#include "bincount_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace jk;

static void need(bool ok, const char *what, uint64_t a, uint64_t b) {
    if (ok) return;
    std::fprintf(stderr, "bincount_plan_check: %s fails at %llu, %llu\n", what, (unsigned long long)a, (unsigned long long)b);
    std::exit(1);
}

static uint64_t cases = 0;

static void check_batch(const std::vector<int64_t> &lens, int64_t first, unsigned code_seed) {
    const int64_t n = (int64_t)lens.size();
    std::vector<int64_t> offs((size_t)n + 1);
    std::vector<uint8_t> codes((size_t)n);
    offs[0] = first;
    for (int64_t i = 0; i < n; ++i) {
        offs[i + 1] = offs[i] + lens[i];
        codes[i] = (uint8_t)((i * 7 + code_seed + (i / 40) % 2) % BC_BINS);
        if (code_seed == 9) codes[i] = (uint8_t)((i / 40) % BC_BINS);      // runs of 40 reads of one code
    }
    need(bincount_check(n, offs.data(), codes.data()) == BC_OK, "a proper batch is accepted", (uint64_t)n, code_seed);
    if (n) {
        codes[n / 2] = BC_BINS;
        need(bincount_check(n, offs.data(), codes.data()) == BC_BAD_CODE, "a code of 3", (uint64_t)n, code_seed);
        codes[n / 2] = 255;
        need(bincount_check(n, offs.data(), codes.data()) == BC_BAD_CODE, "a code of 255", (uint64_t)n, code_seed);
        codes[n / 2] = (uint8_t)(code_seed % BC_BINS);
        need(bincount_check(n, offs.data(), nullptr) == BC_BAD_ARGS && bincount_check(n, nullptr, codes.data()) == BC_BAD_ARGS, "missing arrays", (uint64_t)n, code_seed);
        const int64_t keep = offs[n];
        offs[n] = offs[n - 1] - 1;
        need(bincount_check(n, offs.data(), codes.data()) == BC_BAD_OFFSETS, "offsets that decrease", (uint64_t)n, code_seed);
        offs[n] = keep;
        const int64_t keep0 = offs[0];
        offs[0] = -1;
        need(bincount_check(n, offs.data(), codes.data()) == BC_BAD_OFFSETS, "offsets that start below 0", (uint64_t)n, code_seed);
        offs[0] = keep0;
    }
    for (uint32_t mask = 1; mask < (1u << BC_BINS); ++mask) {
        SinkList L;
        sink_list(n, offs.data(), codes.data(), mask, L);
        // the restatement: the selected reads in order, each with its bytes and one separator
        uint64_t reads = 0, at = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (!((mask >> codes[i]) & 1u)) continue;
            need(reads < L.src.size() && L.src[reads] == offs[i] && L.dst[reads] == at, "a read's source and destination", (uint64_t)i, mask);
            at += (uint64_t)lens[i] + 1;
            ++reads;
        }
        need(L.reads == reads && L.src.size() == reads && L.dst.size() == reads + 1 && L.dst[reads] == at && L.bases == at - reads, "a list's totals", reads, mask);
        for (uint64_t piece : {(uint64_t)1, (uint64_t)16, (uint64_t)17, (uint64_t)256, (uint64_t)4096, BC_PIECE}) {
            uint64_t j0 = 0, most = 0;
            while (j0 < reads) {
                const uint64_t j1 = piece_end(L.dst, j0, piece);
                need(j1 > j0 && j1 <= reads, "a piece holds at least one read and ends inside the list", j0, piece);
                const uint64_t bytes = L.dst[j1] - L.dst[j0];
                need(bytes <= piece || j1 == j0 + 1, "a piece above the piece size is one read", j0, piece);
                need(j1 == reads || L.dst[j1 + 1] - L.dst[j0] > piece, "a piece takes every read that fits", j0, piece);
                need(piece_room(bytes) >= bytes + BC_PAD && piece_room(bytes) % BC_GROUP == 0 && piece_groups(bytes) * BC_GROUP == piece_room(bytes) &&
                         piece_blocks(bytes) * BC_THREADS >= piece_groups(bytes),
                     "a piece's buffer and launch", bytes, piece);
                most = bytes > most ? bytes : most;
                j0 = j1;
            }
            need(largest_piece(L.dst, piece) == most, "the largest piece", most, piece);
            ++cases;
        }
    }
}

int main() {
    check_batch({}, 0, 0);
    for (int64_t one : {0, 1, 15, 16, 17, 255, 256, 257, 70000}) check_batch({one}, 3, 1);
    check_batch({0, 0, 0}, 0, 2);
    check_batch({1, 15, 16, 17, 0, 0, 1}, 5, 0);
    check_batch({300, 100000, 300, 0, 300}, 1, 1);
    {
        std::vector<int64_t> lens;
        for (int i = 0; i < 400; ++i) lens.push_back((int64_t)((i * 37) % 260));
        lens[200] = 70000;
        for (unsigned seed : {0u, 1u, 2u, 9u}) check_batch(lens, 15, seed);
    }
    // the masks and the limits: refused by their value alone, before an array is looked at
    need(!bincount_mask_ok(0) && !bincount_mask_ok(8) && !bincount_mask_ok(0xFFFFFFFFu) && bincount_mask_ok(1) && bincount_mask_ok(7), "masks", 0, 0);
    const int64_t zero = 0;
    need(bincount_check(BC_MAX_READS + 1, &zero, nullptr) == BC_TOO_LARGE, "2^31 reads", 0, 0);
    need(bincount_check(-1, &zero, nullptr) == BC_BAD_ARGS, "a negative read count", 0, 0);
    const int64_t far[2] = {0, BC_MAX_TEXT + 1};
    const uint8_t code0 = 0;
    need(bincount_check(1, far, &code0) == BC_TOO_LARGE, "more than 2^43 text bytes", 0, 0);
    need(piece_room((uint64_t)BC_MAX_TEXT + 1) > (uint64_t)BC_MAX_TEXT && piece_blocks(BC_PIECE_MOST) <= 0x7FFFFFFFull, "the largest sizes do not wrap", 0, 0);
    // the piece hook
    uint64_t piece = 0;
    need(piece_from_text("256", piece) && piece == 256 && piece_from_text("68719476736", piece) && piece == BC_PIECE_MOST, "piece sizes that are accepted", 0, 0);
    for (const char *bad : {"", "0", "x", "12x", "-1", "68719476737", "99999999999999999999999999"})
        need(!piece_from_text(bad, piece), "a piece size that is refused", 0, 0);
    need(!piece_from_text(nullptr, piece), "no piece size", 0, 0);
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
