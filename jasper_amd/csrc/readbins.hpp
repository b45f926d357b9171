// readbins.hpp -- trio read binning: per read of a packed batch, how many of its windows hold a k-mer that only the mother's reads have
// and how many hold one that only the father's have (readbins.hip).
//
// An extension: the reference has no counterpart.  The hap-mer scan's two probes per window (hapmers.hip, no child table) over READS
// instead of contigs: the work is cut over the packed text, not per read, and a read's two counters are all that comes back.
// Semantics: include/jasper_hip.h (jasper_read_bins).  The binning rule and the files are host work: jasper_amd/triobin.py.
#pragma once
#include "report.hpp"
#include <string>

namespace jk {

// What the index arithmetic allows (more is refused with a message):
//   reads per call     a read's index is an int in the searches of the offsets
//   text bytes         a tile's index is 32 bits (ScanTile::idx) and a tile is RP_TILE windows; 2^43 leaves every byte position and every
//                      start-bit word index far inside 64 bits
//   windows per read   a read's counters are 32 bits and are added to, not clamped
constexpr int64_t RB_MAX_READS = 0x7FFFFFFF;
constexpr int64_t RB_MAX_TEXT = (int64_t)1 << 43;
constexpr int64_t RB_MAX_READ_WINDOWS = 0xFFFFFFFFll;

// read i = d_text[offsets[i] .. offsets[i+1]) on the tables' device; offsets is a host array of n_reads + 1 entries; out_mat / out_pat are
// host arrays of n_reads words.  seconds (may be null) = device time (HIP events) of the start-bit pass and the scan.
int read_bins_device(Table &M, Table &P, int64_t n_reads, const uint8_t *d_text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t *out_mat,
                     uint32_t *out_pat, double *seconds, std::string &err);
// what both run, and the read-text path on its packed sequences (readtext.hip): n_reads > 0 reads of L bytes in all whose offsets are
// either a host array (h_offs: uploaded) or in HBM already (d_offs_in: the n_reads + 1 offsets, then {offsets[0], offsets[n_reads]}).
// Nothing is checked and nothing is waited for: the counters stay on the device (*d_cnt_out: mat[n_reads], pat[n_reads]) and ev holds
// the two events around the kernels.
struct Events;
int read_bins_core(Table &M, Table &P, int64_t n_reads, const uint8_t *d_text, const int64_t *h_offs, const int64_t *d_offs_in, int64_t L, uint32_t thre_mat, uint32_t thre_pat,
                   Events &ev, uint32_t **d_cnt_out, std::string &err);
// the same with the text in host memory: the bytes text[offsets[0] .. offsets[n_reads]) are uploaded
int read_bins_host(Table &M, Table &P, int64_t n_reads, const char *text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t *out_mat, uint32_t *out_pat,
                   double *seconds, std::string &err);

}  // namespace jk
