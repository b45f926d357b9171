// bincount.hpp -- the reads of chosen bins of a packed batch counted into tables of their own (bincount.hip).
//
// An extension: the reference has no counterpart.  The read binning (readbins.hip) says which bin a read belongs to; this makes the
// k-mer table of "the reads of bins {..}" while the batch is in HBM, so that a haplotype can be polished from a database of its own
// reads without those reads being written to disk and counted again.  Up to three SINKS a call: a sink is a destination table and a
// 3-bit mask of the bin codes it takes.  A sink's reads are gathered, in input order and each followed by one separator byte, into
// the stream Table::count_device takes, piece by piece of whole reads (bincount_plan.hpp), and counted there by that call -- the
// counting kernels are the tables' own.  Semantics: include/jasper_hip.h (jasper_count_binned).
#pragma once
#include "bincount_plan.hpp"
#include "table.hpp"
#include <string>

namespace jk {

struct BinSinks {
    int n = 0;                  // 1 .. BC_SINKS
    Table *const *tables = nullptr;
    const uint32_t *masks = nullptr;
    uint64_t *out = nullptr;    // per sink: reads, bases, k-mer occurrences gathered
    double *seconds = nullptr;  // per sink (may be null): device time of the gather kernel (HIP events), wall time of the counting calls
};

// read i = d_text[offsets[i] .. offsets[i + 1]) on the sinks' device, at any alignment; offsets (n_reads + 1) and codes (n_reads) are
// host arrays.  `keep` (may be null): tables that may not be sinks (the binning's own), named in the refusal
int count_binned_device(const BinSinks &S, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, const uint8_t *codes, Table *const *keep, int n_keep, std::string &err);
// the same with the text in host memory: text[offsets[0] .. offsets[n_reads]) is uploaded into the first sink's workspace
int count_binned_host(const BinSinks &S, int64_t n_reads, const char *text, const int64_t *offsets, const uint8_t *codes, std::string &err);
// ... and with the packed sequences and offsets the last read-text call on M left in M's workspace (readtext.hip): no sequence visits
// the host.  Refused when n_records is not what that call returned.  P (may be null) is the binning's other table
int read_text_count(Table &M, Table *P, int64_t n_records, const uint8_t *codes, const BinSinks &S, std::string &err);

}  // namespace jk
