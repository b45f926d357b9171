// readtext.hpp -- the child's read files parsed and packed on the GPU for the trio read binning (readtext.hip).
//
// An extension: the reference has no counterpart.  A chunk of raw FASTQ / FASTA text is uploaded as it stands; kernels find its lines,
// verify the record shape, pack the sequences back to back and write the n + 1 offsets read_bins_kernel takes, so that only the small
// per-record arrays travel back.  What the kernels produce is what the host parser of jasper_amd/triobin.py (_lines, _without_cr,
// _fastq_chunk, _fasta_chunk) produces for the same (text, eof).  Semantics: include/jasper_hip.h (jasper_read_text_bins).
#pragma once
#include "readtext_plan.hpp"
#include "report.hpp"
#include <string>

namespace jk {

// Upload, index, pack and bin one chunk: text[0 .. n) in host memory, its first byte a record's first.  used = the bytes whole records
// cover, n_records = how many; status RT_CLEAN or RT_MALFORMED with bad_record = the first record that fails a check (n_records when the
// file ends inside a record); on RT_MALFORMED nothing is binned.  seconds[0] = device time of index + pack, seconds[1] = of the start
// bits and the scan (HIP events).  The results stay in M's workspace for read_text_fetch.
int read_text_bins(Table &M, Table &P, const char *text, int64_t n, int eof, int format, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status,
                   int64_t *bad_record, double *seconds, std::string &err);
// The same for text that is already in HBM: text[0 .. n) lies at the front of M's workspace slot WS_READTEXT, which has n + RT_PAD bytes.
// last_is_lf says whether text[n - 1] is a line feed (the one thing the host stage has to know of the text itself): 1, 0, or -1 for "read
// that byte from the device", a one-byte copy queued with the line-feed total the stage waits for anyway.  The caller has run
// read_text_check (with this n, or with 0 and an n of its own below 2^31) on the same outputs.  read_text_bins is that check, its upload
// and this.
int read_text_core(Table &M, Table &P, int64_t n, int eof, int format, int last_is_lf, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status,
                   int64_t *bad_record, double *seconds, std::string &err);
// what both refuse before the text is looked at (tables, thresholds, n, format), and the outputs' initial state
int read_text_check(Table &M, Table &P, int64_t n, int format, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status, int64_t *bad_record,
                    double *seconds, std::string &err);
// out[i] = the sum of in[0 .. i) for i <= n (n + 1 words) on stream st, by the scan kernels of the line scan; blk: rt_blocks(n) + 1 words
int rt_scan_words(hipStream_t st, const uint64_t *d_in, uint64_t n, uint64_t *d_blk, uint64_t *d_out, std::string &err);
// what the call before left: rec_start[n_records + 1] (the last = used), head_end[n_records], lens[n_records], the two counters per
// record, and (out_seq not null) the packed sequences, sum of lens bytes.  Refused when n_records is not what that call returned.
int read_text_fetch(Table &M, int64_t n_records, int64_t *rec_start, int64_t *head_end, int64_t *lens, uint32_t *out_mat, uint32_t *out_pat, uint8_t *out_seq, std::string &err);

}  // namespace jk
