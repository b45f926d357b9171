// report.hpp -- dense k-mer report of a set of sequences against the resident table (report.hip).
//
// An extension: the reference has no counterpart.  It takes the windows of src/jasper.py:55-71 DENSELY (every window of
// every sequence, not the strided walk of the QV pass) and hands back per-sequence counters and the maximal runs of
// unreliable windows.
#pragma once
#include "table.hpp"
#include <string>
#include <vector>

namespace jk {

constexpr int RP_THREADS = 256, RP_GROUP = 16, RP_TILE = RP_THREADS * RP_GROUP, RP_HALO = 4;   // RP_TILE windows per workgroup iteration

// a maximal run of unreliable windows (layout of the public jasper_kmer_run)
struct KmerRun {
    int64_t start;
    uint64_t n_kmers;
    uint64_t n_absent;
    uint32_t seq;
    uint32_t min_count;
};

struct ReportOut {
    std::vector<uint64_t> counts;   // 4 per sequence: windows, valid, unreliable, absent
    std::vector<KmerRun> runs;      // ordered by (seq, start)
    double seconds = 0;             // device time (HIP events) of the kernels
    int retried = 0;                // the scan was repeated with a larger buffer for the partial runs
};

// sequence i = d_text[offsets[i] .. offsets[i+1]) on the table's device; offsets is a host array of n_seqs + 1 entries
int kmer_report_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, ReportOut &R, std::string &err);
int kmer_report_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, ReportOut &R, std::string &err);

}  // namespace jk
