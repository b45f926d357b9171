// deflate_plan.hpp -- the host arithmetic of the device compressor (deflate_gpu.hip): how a text is cut into BGZF blocks, how large the
// members can get and how large every buffer of the path is.  Plain C++, no HIP: tools/deflate_plan_check.cpp runs it under
// -fsanitize=address,undefined.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jk {

constexpr int DF_BLOCK = 65280;                 // text bytes of one member at the most (the SAM specification's bound for a BGZF block)
constexpr int DF_MEMBER_MOST = 65536;           // bytes of one member at the most (BSIZE is 16 bits)
constexpr int DF_HEAD = 18, DF_TAIL = 8;        // a member's header, and its CRC-32 and ISIZE
constexpr int DF_STORED = 5;                    // BFINAL / BTYPE byte, LEN, NLEN of the one stored block a member may fall back to
constexpr int DF_FRAME = DF_HEAD + DF_TAIL + DF_STORED;      // 31: what a member adds to its text at the most
constexpr int DF_SLOT = DF_MEMBER_MOST;         // bytes of a member's slot in the staging buffer the compress kernel writes
constexpr int DF_AUX_WORDS = DF_BLOCK / 3;      // a block's match records: one word per three positions (two matches begin >= 3 apart)
constexpr int DF_COUNTERS = 6;                  // blocks, stored, literal-only and LZ blocks, matches, matched bytes
constexpr int64_t DF_MAX_TEXT = 0x7FFFFFFF;     // text bytes per call
constexpr int DF_PAD = 64;                      // bytes behind the text and behind the packed members (16-byte loads and stores end inside)
static_assert(DF_BLOCK + DF_FRAME <= DF_MEMBER_MOST, "a stored member fits");
static_assert(DF_BLOCK % 3 == 0, "the match records' slots");

enum { DF_OK = 0, DF_TOO_LARGE = 1 };
inline int deflate_check(int64_t n) { return n < 0 || n > DF_MAX_TEXT ? DF_TOO_LARGE : DF_OK; }

inline uint64_t deflate_blocks(uint64_t n) { return (n + DF_BLOCK - 1) / DF_BLOCK; }
// text bytes of block b of a text of n bytes (b < deflate_blocks(n))
inline uint32_t deflate_block_bytes(uint64_t n, uint64_t b) { return (uint32_t)(n - b * DF_BLOCK < (uint64_t)DF_BLOCK ? n - b * DF_BLOCK : (uint64_t)DF_BLOCK); }
// what the members of n text bytes come to at the most: every block stored
inline uint64_t deflate_bound(uint64_t n) { return n + (uint64_t)DF_FRAME * deflate_blocks(n); }

// bytes of the path's buffers
struct DeflateBuffers {
    size_t text = 0;        // the text of a host call, up to 15 bytes before it (it keeps its host pointer's place within 16 bytes) and its padding
    size_t slots = 0;       // a slot per block: the member as the compress kernel leaves it
    size_t aux = 0;         // a block's match records
    size_t sizes = 0;       // uint64 per block: the member's bytes
    size_t pre = 0;         // their exclusive scan with the total behind it
    size_t scan_blocks = 0; // uint64 per block of that scan and one for the total (scan_elems = elements of one scan block)
    size_t out = 0;         // the members back to back
};
inline DeflateBuffers deflate_buffers(uint64_t n, uint64_t scan_elems) {
    const uint64_t nb = deflate_blocks(n), some = nb ? nb : 1;      // (no buffer is empty: a kernel or a scan is handed a pointer)
    DeflateBuffers b;
    b.text = (size_t)n + 15 + DF_PAD;
    b.slots = (size_t)some * DF_SLOT;
    b.aux = (size_t)some * DF_AUX_WORDS * sizeof(uint32_t);
    b.sizes = (size_t)some * sizeof(uint64_t);
    b.pre = (size_t)(nb + 1) * sizeof(uint64_t);
    b.scan_blocks = (size_t)((nb + scan_elems - 1) / scan_elems + 1) * sizeof(uint64_t);
    b.out = (size_t)deflate_bound(n) + DF_PAD;
    return b;
}

}  // namespace jk
