// compound.hpp -- compound scan of a set of sequences against the resident read table (compound.hip).
//
// An extension: what the reads hold in place of a CLUSTER of differences.  Two differences less than k apart hide each other from the
// variant and the indel scan -- no single-edit alternative is solid -- and leave a run of unreliable windows of k + R - 1 windows, R the
// bytes from the first difference to the last.  The dense report (report.hpp) finds those runs unchanged; a search kernel then walks
// the solid k-mers of the reads from the run's left flank and lists every string that rejoins the sequence on its right flank
// (semantics: include/jasper_hip.h, jasper_compound_scan).  With no site nothing of the search is allocated or launched.
#pragma once
#include "report.hpp"

namespace jk {

constexpr int COMPOUND_MAX_LEN = 64;
constexpr int COMPOUND_FRONT = 64;      // the search keeps at most this many prefixes of one length (JASPER_COMPOUND_FRONT = JASPER_INDEL_FRONT)

// where a search starts and ends: the R = q - a bytes s[a .. q) of sequence seq are what is replaced; ref_min is copied into the records
struct CompoundSite {
    int64_t a, q;
    uint32_t seq, ref_min;
};
static_assert(sizeof(CompoundSite) == 24, "uploaded as it is");

// a replacement the reads hold (layout of the public jasper_compound)
struct Compound {
    int64_t pos;                   // a
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint32_t ref_len;              // R
    uint64_t bases[2];             // base i of y in bits 2i, 2i + 1 (of bases[i / 32]); 0 above 2 * len
    uint16_t len;
    uint8_t pad[6];
};
static_assert(sizeof(Compound) == 48, "layout of jasper_compound");

struct CompoundOut {
    std::vector<uint64_t> counts;    // 5 per sequence: sites, bridged, records, long, complex
    std::vector<Compound> recs;      // ordered by (seq, pos, len, y)
    double seconds = 0;              // device time (HIP events) of the dense scan and the search
    double search_seconds = 0;       // ... of compound_search_kernel alone
    uint64_t lookups = 0;            // table lookups it made (its last run)
    int retried = 0;                 // it was repeated with a larger record list
};

// `report` gets what kmer_report_device gives on the same input: the one dense scan of the call (the only copy of it)
int compound_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, ReportOut &report, CompoundOut &out,
                         std::string &err);
int compound_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, ReportOut &report, CompoundOut &out,
                       std::string &err);

}  // namespace jk
