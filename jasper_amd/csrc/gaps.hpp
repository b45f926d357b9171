// gaps.hpp -- gap scan of a set of sequences against the resident read table (gaps.hip).
//
// An extension: a Sealer-style closure of scaffold gaps (runs of non-base bytes, which no other scan here sees: a window that holds one
// has no k-mer) and, when asked for, of the runs of unreliable k-mers that the compound scan counts as `long`.  The dense report
// (report.hpp) finds the unreliable runs unchanged, gap_runs_kernel the runs of windows without a k-mer; the host makes the sites from
// the two lists (gaps_host.hpp), and a search kernel walks the solid k-mers of the reads from each site's left flank until they rejoin
// its right flank, for up to GAP_MAX_LEN levels: the path is not kept in registers but in a per-wave log in global memory (semantics:
// include/jasper_hip.h, jasper_gap_scan).  With no site to search nothing of the search is allocated or launched.
#pragma once
#include "gaps_host.hpp"
#include "report.hpp"

namespace jk {

// a maximal run of windows that hold a non-base byte
struct GapRun {
    int64_t start;
    uint64_t n_kmers;
    uint32_t seq;
    uint32_t pad;
};

struct GapOut {
    std::vector<uint64_t> counts;    // GAP_COUNTS per sequence: sites, searched, bridged, unique, records, edge, ragged, limit, complex
    std::vector<GapSite> sites;      // ordered by (seq, a)
    std::vector<GapFill> fills;      // ordered by (seq, pos, len, y); bases_off in that order too
    std::vector<char> pool;          // the fills' bases, upper case
    double seconds = 0;              // device time (HIP events) of the dense scan, the runs scan and the search
    double runs_seconds = 0;         // ... of gap_runs_kernel and its stitch kernels
    double search_seconds = 0;       // ... of gap_search_kernel alone
    uint64_t lookups = 0;            // table lookups it made (its last run)
    int retried = 0;                 // it was repeated with a larger record list or byte pool
};

// `report` gets what kmer_report_device gives on the same input: the one dense scan of the call
int gap_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, int64_t max_trim, bool long_runs, ReportOut &report,
                    GapOut &out, std::string &err);
int gap_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int64_t max_trim, bool long_runs, ReportOut &report,
                  GapOut &out, std::string &err);
// the search alone on a caller's sites: a, q, seq and ref_min of each are read (gap_check_sites)
int gap_search_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, const GapSite *sites, uint64_t n_sites, GapOut &out,
                      std::string &err);
int gap_search_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, const GapSite *sites, uint64_t n_sites, GapOut &out,
                    std::string &err);

}  // namespace jk
