// deflate_plan_check.cpp -- jasper_amd/csrc/deflate_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -fsanitize=address,undefined -Ijasper_amd/csrc tools/deflate_plan_check.cpp -o deflate_plan_check && ./deflate_plan_check
//
// No HIP, no GPU.  It walks the text lengths at which the compressor's arithmetic changes -- none, one byte, a block less one, a block,
// a block and one, several blocks, the largest call -- and checks the number of blocks, that the blocks' bytes add up to the text and none
// is empty or too long, the output bound, the refusals, and that every buffer holds what the kernels index: heap arrays of exactly the
// planned size are written at the last place each kernel reaches; `ok` at the end.
#include "deflate_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace jk;

static void need(bool ok, const char *what, uint64_t n) {
    if (ok) return;
    std::fprintf(stderr, "deflate_plan_check: %s fails at n = %llu\n", what, (unsigned long long)n);
    std::exit(1);
}

static uint64_t cases = 0;
constexpr uint64_t SCAN = 4096;     // elements of one block of the scan the path uses (RT_BLOCK)

static void check_n(uint64_t n, bool touch) {
    const uint64_t nb = deflate_blocks(n);
    need(deflate_check((int64_t)n) == DF_OK, "a text below 2^31 bytes is taken", n);
    need(nb == n / DF_BLOCK + (n % DF_BLOCK ? 1 : 0), "the number of blocks", n);
    need((n == 0) == (nb == 0), "no text, no block", n);
    uint64_t sum = 0;
    for (uint64_t b = 0; b < nb; b += (nb > 64 && b + 2 < nb && b >= 2) ? nb - 4 : 1) {      // (the first and the last blocks of a long text)
        const uint32_t bytes = deflate_block_bytes(n, b);
        need(bytes >= 1 && bytes <= (uint32_t)DF_BLOCK, "a block holds 1 .. 65280 bytes", n);
        need((b + 1 < nb) == (bytes == (uint32_t)DF_BLOCK && (b + 1) * DF_BLOCK < n), "only the last block is short", n);
        need(bytes + DF_FRAME <= (uint32_t)DF_MEMBER_MOST && bytes + DF_FRAME <= (uint32_t)DF_SLOT, "a stored member fits BSIZE and its slot", n);
        need((bytes - 1) / 3 < (uint32_t)DF_AUX_WORDS, "a match record's word lies in the block's records", n);
        if (nb <= 64) sum += bytes;
    }
    if (nb <= 64) need(sum == n, "the blocks add up to the text", n);
    need(deflate_bound(n) == n + 31 * nb && deflate_bound(n) >= n, "the bound is n + 31 per block", n);
    const DeflateBuffers B = deflate_buffers(n, SCAN);
    need(B.text >= n + 15 + 16 && B.out >= deflate_bound(n) + 16, "room around the text and behind the members", n);
    need(B.slots >= nb * (uint64_t)DF_SLOT && B.slots >= (uint64_t)DF_SLOT && B.aux >= nb * DF_AUX_WORDS * 4 && B.aux > 0, "slots and match records", n);
    need(B.sizes >= nb * 8 && B.sizes >= 8 && B.pre == (nb + 1) * 8, "sizes and their scan", n);
    need(B.scan_blocks == ((nb + SCAN - 1) / SCAN + 1) * 8, "scan blocks", n);
    if (touch) {                    // the last byte or word each kernel can reach, in arrays of exactly the planned size
        std::vector<uint8_t> slots(B.slots), out(B.out);
        std::vector<uint8_t> aux(B.aux), sizes(B.sizes), pre(B.pre);
        if (nb) {
            const uint32_t last = deflate_block_bytes(n, nb - 1);
            slots[(nb - 1) * DF_SLOT + last + DF_FRAME - 1] = 1;                    // a stored member's ISIZE
            slots[(nb - 1) * DF_SLOT + ((last + DF_FRAME + 3) / 4) * 4 - 1] = 1;    // ... and the word a bit writer ends in
            aux[((nb - 1) * DF_AUX_WORDS + (last - 1) / 3) * 4 + 3] = 1;
            sizes[(nb - 1) * 8 + 7] = 1;
            out[deflate_bound(n) - 1 + 15] = 1;                                     // a 16-byte store that begins at the last byte
        }
        pre[nb * 8 + 7] = 1;
    }
    ++cases;
}

int main() {
    const uint64_t K = DF_BLOCK;
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 17, 64 * K, 64 * K + 1, SCAN * K, SCAN * K + 1}) check_n(n, n <= 64 * K + 1);
    check_n((uint64_t)DF_MAX_TEXT, false);
    need(deflate_blocks((uint64_t)DF_MAX_TEXT) == 32897, "the largest call's blocks", (uint64_t)DF_MAX_TEXT);
    need(deflate_buffers((uint64_t)DF_MAX_TEXT, SCAN).slots == 32897ull * DF_SLOT, "the largest call's sizes do not wrap", (uint64_t)DF_MAX_TEXT);
    // the refusals
    need(deflate_check(DF_MAX_TEXT + 1) == DF_TOO_LARGE, "a text of 2^31 bytes is refused", (uint64_t)DF_MAX_TEXT + 1);
    need(deflate_check(-1) == DF_TOO_LARGE, "a negative length is refused", 0);
    need(deflate_check(INT64_MAX) == DF_TOO_LARGE && deflate_check(INT64_MIN) == DF_TOO_LARGE, "the ends of int64 are refused", 0);
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
