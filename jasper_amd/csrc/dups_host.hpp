// dups_host.hpp -- the host side of the duplication map (dups.hip): the run record and what turns the device's form of a run into the
// public one.  Plain C++, nothing of HIP, so that tools/dups_host_check.cpp can build it alone.
//
// On the device a run carries in mate_start the GLOBAL position (offsets[seq] + window) of the mate of its FIRST window, and nothing in
// mate_seq.  The mate stretch of a `+` run ascends from there, that of a `-` run descends, so its leftmost window is the mate of the run's
// last window.  The public form has the leftmost window of the mate stretch, as (sequence, window in that sequence).  For k >= 2 the mate
// stretch lies in one sequence: the last window of a sequence and the first of the next one are k positions apart, never one.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace jk {

// a maximal colinear run of two-copy windows (layout of the public jasper_dup_run)
struct DupRun {
    int64_t start;          // first window, in sequence seq
    int64_t mate_start;     // leftmost window of the mate stretch, in sequence mate_seq (device: see above)
    uint64_t n_kmers;
    uint64_t sum_reads;
    uint64_t n_deficit;
    uint32_t seq;
    uint32_t mate_seq;
    uint32_t strand;        // 0: `+`, the mates ascend with the run; 1: `-`, they descend
    uint32_t pad;
};
static_assert(sizeof(DupRun) == 56, "layout of jasper_dup_run");

// a position's encoding in the side array: the position and the strand bit of the window there
inline uint64_t dup_encode(int64_t gpos, uint32_t strand) { return ((uint64_t)gpos << 1) | (strand & 1u); }

// the sequence that holds global position g: the last one that starts at or before it (empty sequences before it start there too, and
// are passed over)
inline int dup_seq_of(int64_t g, int n_seqs, const int64_t *offsets) {
    return (int)(std::upper_bound(offsets, offsets + n_seqs, g) - offsets) - 1;
}

// the device's runs made public, in place; -1 and a message when a mate stretch does not lie inside one sequence's windows (the tables
// or the offsets are not what the scan was given)
inline int dup_finish_runs(std::vector<DupRun> &runs, int k, int n_seqs, const int64_t *offsets, std::string &err) {
    for (DupRun &r : runs) {
        const int64_t left = r.strand ? r.mate_start - (int64_t)(r.n_kmers - 1) : r.mate_start;
        const int s = left >= 0 && n_seqs > 0 ? dup_seq_of(left, n_seqs, offsets) : -1;
        if (s < 0 || left + (int64_t)r.n_kmers - 1 + k > offsets[s + 1]) {
            err = "duplication map: a run's mates do not lie in one sequence";
            return -1;
        }
        r.mate_seq = (uint32_t)s;
        r.mate_start = left - offsets[s];
        r.pad = 0;
    }
    return 0;
}

}  // namespace jk
