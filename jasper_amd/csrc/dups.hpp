// dups.hpp -- duplication map of a set of sequences against two resident tables, the reads' and the assembly's (dups.hip).
//
// An extension: the reference has no counterpart.  The copy scan says where the assembly holds a k-mer more often than the reads support;
// this pairs every window whose k-mer the assembly holds exactly twice with the place of the other copy and hands back the maximal
// colinear runs of such pairs (semantics: include/jasper_hip.h, jasper_dup_map).
#pragma once
#include "dups_host.hpp"
#include "report.hpp"
#include <string>
#include <vector>

namespace jk {

struct DupOut {
    std::vector<uint64_t> counts;   // 7 per sequence: windows, valid, two_copy, deficit, multi, unplaced, sum_reads
    std::vector<DupRun> runs;       // ordered by (seq, start)
    double index_seconds = 0;       // device time (HIP events) of the side array's fill and dup_index_kernel
    double seconds = 0;             // ... of dup_scan_kernel (both attempts if it was repeated) and the two stitch kernels
    int retried = 0;                // the scan was repeated with a larger buffer for the partial runs
};

// sequence i = d_text[offsets[i] .. offsets[i+1]) on the tables' device; offsets is a host array of n_seqs + 1 entries
int dup_map_device(Table &R, Table &A, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak, DupOut &out, std::string &err);
int dup_map_host(Table &R, Table &A, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak, DupOut &out, std::string &err);

}  // namespace jk
