// diploid.hpp -- both haplotypes of a diploid assembly against the reads (diploid.hip): the join of three resident tables (reads R,
// assembly A1, other haplotype A2) into the pair spectrum, and the dense scan of one haplotype's sequences against R and the OTHER
// haplotype's table.
//
// An extension: the reference has no counterpart.  Semantics: include/jasper_hip.h (jasper_table_spectrum_pair, jasper_pair_scan).
#pragma once
#include "report.hpp"
#include "spectra.hpp"
#include <string>
#include <vector>

namespace jk {

constexpr int SPP_ROWS = 4;         // (key in A1 ? 1 : 0) | (key in A2 ? 2 : 0): reads only, asm only, alt only, shared

enum { PS_NONE = 0, PS_SOLID = 1, PS_WEAK = 2 };   // class of a window / kind of a run: private and solid, private and weak

// a maximal run of windows of one class (layout of the public jasper_pair_run)
struct PairRun {
    int64_t start;
    uint64_t n_kmers;
    uint64_t sum_reads;
    uint32_t seq;
    uint32_t kind;
};
static_assert(sizeof(PairRun) == 32, "layout of jasper_pair_run");

struct PairOut {
    std::vector<uint64_t> counts;   // 6 per sequence: windows, valid, unreliable, absent, private_solid, private_weak
    std::vector<PairRun> runs;      // ordered by (seq, start)
    double seconds = 0;             // device time (HIP events) of the kernels
    int retried = 0;                // the scan was repeated with a larger buffer for the partial runs
};

// out: SPP_ROWS * SP_COLS cells, row-major (host memory); seconds: device time (HIP events) of the three sweeps
int table_spectrum_pair(Table &R, Table &A1, Table &A2, uint64_t *out, double *seconds, std::string &err);

// sequence i = seqs[i][0 .. lens[i]) in host memory
int pair_scan_host(Table &R, Table &O, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, PairOut &out, std::string &err);

}  // namespace jk
