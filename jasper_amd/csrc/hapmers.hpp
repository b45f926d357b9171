// hapmers.hpp -- trio hap-mer scan and census: the k-mers only one parent's reads hold, located on a set of sequences and counted
// against an assembly's table (hapmers.hip).
//
// An extension: the reference has no counterpart.  The dense scan of copies.hip with three tables (mother M, father P, child R) and the
// slot sweep of spectra.hip with four (M, P, R and the assembly A).  Semantics: include/jasper_hip.h (jasper_hapmer_scan,
// jasper_hapmer_census).  The phase blocks made from the runs are host work: jasper_amd/hapmers.py.
#pragma once
#include "report.hpp"
#include <string>
#include <vector>

namespace jk {

enum { HM_NONE = 0, HM_MAT = 1, HM_PAT = 2 };          // class of a window / kind of a run

// a maximal run of windows of one class = one marker (layout of the public jasper_hap_run)
struct HapRun {
    int64_t start;
    uint64_t n_kmers;
    uint32_t seq;
    uint32_t kind;
};
static_assert(sizeof(HapRun) == 24, "layout of jasper_hap_run");

struct HapOut {
    std::vector<uint64_t> counts;   // 4 per sequence: windows, valid, mat, pat
    std::vector<HapRun> runs;       // ordered by (seq, start)
    double seconds = 0;             // device time (HIP events) of the kernels
    int retried = 0;                // the scan was repeated with a larger buffer for the partial runs
};

// R may be null (no inheritance filter).  sequence i = d_text[offsets[i] .. offsets[i+1]) on the tables' device; offsets is a host
// array of n_seqs + 1 entries
int hapmer_scan_device(Table &M, Table &P, Table *R, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                       HapOut &out, std::string &err);
int hapmer_scan_host(Table &M, Table &P, Table *R, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                     HapOut &out, std::string &err);
// out6 = hapmers, found, occurrences of the mother's hap-mers, then of the father's; R and A may be null
int hapmer_census(Table &M, Table &P, Table *R, Table *A, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child, uint64_t out6[6], double *seconds, std::string &err);

// The checks every trio call makes before it touches a table: one k, one device, no handle twice, M, P and A whole tables, thresholds of at
// least 1.  `what` starts the message.  (Hidden: the library's list of exported symbols stays what it was.)
__attribute__((visibility("hidden"))) int check_trio(const char *what, Table &M, Table &P, Table *R, Table *A, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                                                     std::string &err);

}  // namespace jk
