// copies.hpp -- copy-number scan of a set of sequences against two resident tables, the reads' and the assembly's (copies.hip).
//
// An extension: the reference has no counterpart.  The dense scan of report.hip joined with the two tables of spectra.hip: every
// window is looked up in both, classified by the copy number the reads support against the copies the assembly holds, and handed
// back as per-sequence counters and the maximal runs of each class (semantics: include/jasper_hip.h, jasper_copy_report).
#pragma once
#include "report.hpp"
#include <string>
#include <vector>

namespace jk {

enum { CP_NONE = 0, CP_EXCESS = 1, CP_DEFICIT = 2 };   // class of a window / kind of a run

// a maximal run of windows of one class (layout of the public jasper_copy_run)
struct CopyRun {
    int64_t start;
    uint64_t n_kmers;
    uint64_t sum_reads;
    uint64_t sum_asm;
    uint32_t seq;
    uint32_t kind;
};
static_assert(sizeof(CopyRun) == 40, "layout of jasper_copy_run");

struct CopyOut {
    std::vector<uint64_t> counts;   // 6 per sequence: windows, valid, excess, deficit, sum_reads, sum_asm
    std::vector<CopyRun> runs;      // ordered by (seq, start)
    double seconds = 0;             // device time (HIP events) of the kernels
    int retried = 0;                // the scan was repeated with a larger buffer for the partial runs
};

// sequence i = d_text[offsets[i] .. offsets[i+1]) on the tables' device; offsets is a host array of n_seqs + 1 entries
int copies_report_device(Table &R, Table &A, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak, CopyOut &out, std::string &err);
int copies_report_host(Table &R, Table &A, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak, CopyOut &out, std::string &err);

}  // namespace jk
