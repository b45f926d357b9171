// readtext_plan.hpp -- the host arithmetic of the read-text path (readtext.hip): how many lines and records a chunk of raw FASTQ / FASTA
// text holds once its line feeds are counted, and how large every buffer of the path is.  Plain C++, no HIP: tools/readtext_plan_check.cpp
// runs it under -fsanitize=address,undefined.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jk {

constexpr int RT_THREADS = 256;
constexpr int RT_BLOCK = RT_THREADS * 16;       // text bytes of a workgroup, and elements of one block of the line scan
constexpr int RT_SCAN_PASS = 1024;              // block totals that one pass of rt_scan_tops_kernel takes; more are taken in further passes
constexpr int64_t RT_MAX_TEXT = 0x7FFFFFFF;     // text bytes per call: positions and sums of lengths are 32 bits in the kernels
constexpr int RT_PAD = 64;                      // bytes behind the text and behind the packed sequences (16-byte loads and stores end inside)
enum { RT_FASTQ = 0, RT_FASTA = 1 };
enum { RT_CLEAN = 0, RT_MALFORMED = 1 };

// The lines of a chunk of n > 0 bytes with n_lf line feeds.  A line ends at a line feed; at the end of the file a last line without
// one counts.  FASTQ: a record is four lines, a trailing partial record is left, at the end of the file it is malformed.  FASTA: the
// records are counted by the kernels (a header line begins with '>'), every line is looked at.
struct TextLines {
    uint64_t nlines = 0;        // complete lines
    uint64_t nl_use = 0;        // the lines the per-line kernels look at: FASTQ 4 * records, FASTA all
    uint64_t fastq_records = 0;
    bool virtual_end = false;   // the last line ends at n, not at a line feed
    bool ends_inside = false;   // FASTQ at the end of the file: the line count is no multiple of 4
};
inline TextLines text_lines(int format, bool eof, uint64_t n, uint64_t n_lf, bool last_is_lf) {
    TextLines t;
    t.virtual_end = eof && n > 0 && !last_is_lf;
    t.nlines = n_lf + (t.virtual_end ? 1 : 0);
    if (format == RT_FASTQ) {
        t.fastq_records = t.nlines / 4;
        t.ends_inside = eof && t.nlines % 4 != 0;
        t.nl_use = 4 * t.fastq_records;
    } else {
        t.nl_use = t.nlines;
    }
    return t;
}

inline uint64_t rt_blocks(uint64_t elements) { return (elements + RT_BLOCK - 1) / RT_BLOCK; }

// bytes of the buffers that depend on the text and its lines alone
struct TextBuffers {
    size_t text = 0;            // the raw text and its padding
    size_t text_blocks = 0;     // uint64 per text block and one for the total
    size_t nlpos = 0;           // uint32 per line and one more
    size_t line_words = 0;      // uint64 per used line and one for the total (the scan's input needs one less)
    size_t line_blocks = 0;     // uint64 per block of the line scan and one for the total
};
inline TextBuffers text_buffers(uint64_t n, const TextLines &t) {
    TextBuffers b;
    b.text = (size_t)n + RT_PAD;
    b.text_blocks = (size_t)(rt_blocks(n) + 1) * sizeof(uint64_t);
    b.nlpos = (size_t)(t.nlines + 1) * sizeof(uint32_t);
    b.line_words = (size_t)(t.nl_use + 1) * sizeof(uint64_t);
    b.line_blocks = (size_t)(rt_blocks(t.nl_use) + 1) * sizeof(uint64_t);
    return b;
}
// ... and of those that depend on the records: rec_start[n + 1], head_end[n], lens[n] in one buffer of int64; the offsets with the two
// words of the stream's span behind them (readbins.hip: read_bins_kernel)
inline size_t record_words(uint64_t n_records) { return (size_t)(3 * n_records + 1); }
inline size_t offset_words(uint64_t n_records) { return (size_t)(n_records + 3); }

}  // namespace jk
