// readtext_plan_check.cpp -- jasper_amd/csrc/readtext_plan.hpp as a stand-alone program, for a build with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -fsanitize=address,undefined -Ijasper_amd/csrc tools/readtext_plan_check.cpp -o readtext_plan_check && ./readtext_plan_check
//
// No HIP, no GPU.  It walks text sizes and line counts across every boundary the arithmetic has -- a block, a pass of the block-total
// scan, the largest text -- in both formats, with and without the file's end, and checks what must hold of the answers; `ok` at the end.
#include "readtext_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace jk;

static void need(bool ok, const char *what, uint64_t n, uint64_t n_lf) {
    if (ok) return;
    std::fprintf(stderr, "readtext_plan_check: %s fails at n = %llu, n_lf = %llu\n", what, (unsigned long long)n, (unsigned long long)n_lf);
    std::exit(1);
}

int main() {
    const uint64_t sizes[] = {1, 2, 15, 16, 17, RT_BLOCK - 1, RT_BLOCK, RT_BLOCK + 1, (uint64_t)RT_BLOCK * RT_SCAN_PASS - 1, (uint64_t)RT_BLOCK * RT_SCAN_PASS,
                              (uint64_t)RT_BLOCK * RT_SCAN_PASS + 1, (uint64_t)RT_MAX_TEXT - 1, (uint64_t)RT_MAX_TEXT};
    uint64_t cases = 0;
    for (uint64_t n : sizes) {
        const uint64_t lfs[] = {0, 1, 3, 4, 5, RT_BLOCK - 1, RT_BLOCK, RT_BLOCK + 1, n / 2, n - 1, n};
        for (uint64_t n_lf : lfs) {
            if (n_lf > n) continue;
            for (int format = RT_FASTQ; format <= RT_FASTA; ++format)
                for (int eof = 0; eof < 2; ++eof)
                    for (int last_is_lf = 0; last_is_lf < 2; ++last_is_lf) {
                        if ((last_is_lf && n_lf == 0) || (!last_is_lf && n_lf == n)) continue;
                        const TextLines t = text_lines(format, eof != 0, n, n_lf, last_is_lf != 0);
                        need(t.nlines == n_lf + (eof && !last_is_lf ? 1 : 0), "nlines", n, n_lf);
                        need(t.nlines <= n && t.nl_use <= t.nlines, "lines within the text", n, n_lf);
                        need(t.nl_use <= 0x80000000ull, "a line's number fits 32 bits", n, n_lf);
                        if (format == RT_FASTQ) {
                            need(t.nl_use == 4 * t.fastq_records && t.nlines - t.nl_use < 4, "whole FASTQ records", n, n_lf);
                            need(t.ends_inside == (eof && t.nlines % 4 != 0), "ends_inside", n, n_lf);
                        } else {
                            need(t.nl_use == t.nlines && !t.ends_inside, "every FASTA line", n, n_lf);
                        }
                        const TextBuffers b = text_buffers(n, t);
                        need(b.text >= n + 16, "room behind the text", n, n_lf);
                        need(b.text_blocks == (rt_blocks(n) + 1) * 8 && rt_blocks(n) * RT_BLOCK >= n && (rt_blocks(n) - 1) * (uint64_t)RT_BLOCK < n, "text blocks", n, n_lf);
                        need(b.nlpos >= (t.nlines + 1) * 4, "nlpos", n, n_lf);
                        need(b.line_words == (t.nl_use + 1) * 8, "line words", n, n_lf);
                        // the scan's last kernel runs over nl_use + 1 entries: the block that holds the total has a base among the block totals
                        need(rt_blocks(t.nl_use + 1) <= rt_blocks(t.nl_use) + 1 && b.line_blocks >= rt_blocks(t.nl_use + 1) * 8, "line blocks", n, n_lf);
                        const uint64_t most_records = format == RT_FASTQ ? t.fastq_records : t.nlines;
                        need(record_words(most_records) == 3 * most_records + 1 && offset_words(most_records) == most_records + 3, "record words", n, n_lf);
                        need(most_records <= 0x7FFFFFFFull, "records fit the binning's limit", n, n_lf);
                        ++cases;
                    }
        }
    }
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
