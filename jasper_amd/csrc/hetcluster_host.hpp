// hetcluster_host.hpp -- the host side of the het-cluster search (indels.hip, het_cluster_kernel): the record, and what is done with the
// list the kernel leaves -- refuse what it cannot have written, sort, count.  Plain C++ with no HIP in it, so that it also compiles
// into a stand-alone program (tools/hetcluster_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace jk {

constexpr int CLUSTER_MAX_LEN = 64;

// a replacement both of whose sides the reads hold (layout of the public jasper_het_cluster, which is that of jasper_compound)
struct HetCluster {
    int64_t pos;                   // p
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint32_t ref_len;              // R
    uint64_t bases[2];             // base i of y in bits 2i, 2i + 1 (of bases[i / 32]); 0 above 2 * len
    uint16_t len;
    uint8_t pad[6];
};
static_assert(sizeof(HetCluster) == 48, "layout of jasper_het_cluster");

// base i of a record's y
inline unsigned het_cluster_base(const HetCluster &v, int i) { return (unsigned)(v.bases[i >> 5] >> (2 * (i & 31))) & 3u; }

// recs as the kernel left them -> ordered by (seq, pos, ref_len, len, y); counts (4 per sequence: searched, sites, records, complex) gets
// `sites` -- the candidates (pos, y[0]) with a record -- and `records`.  A record the kernel cannot have written is an error.
inline int het_cluster_finish(std::vector<HetCluster> &recs, int n_seqs, int cluster_len, std::vector<uint64_t> &counts, std::string &err) {
    for (const HetCluster &v : recs) {
        bool ok = v.seq < (uint32_t)n_seqs && v.pos >= 0 && v.ref_len >= 1 && v.ref_len <= (uint32_t)cluster_len && v.len >= 1 && (int)v.len <= cluster_len;
        if (ok && v.len < 32) ok = (v.bases[0] >> (2 * v.len)) == 0 && v.bases[1] == 0;
        if (ok && v.len >= 32 && v.len < 64) ok = (v.bases[1] >> (2 * (v.len - 32))) == 0;
        if (!ok) { err = "indel scan: a het cluster the search cannot have written"; return -1; }
    }
    std::sort(recs.begin(), recs.end(), [](const HetCluster &a, const HetCluster &b) {
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.ref_len != b.ref_len) return a.ref_len < b.ref_len;
        if (a.len != b.len) return a.len < b.len;
        for (int i = 0; i < (int)a.len; ++i)
            if (het_cluster_base(a, i) != het_cluster_base(b, i)) return het_cluster_base(a, i) < het_cluster_base(b, i);
        return false;
    });
    unsigned firsts = 0;                                // the first bases seen at the current (seq, pos): one candidate each
    for (size_t i = 0; i < recs.size(); ++i) {
        const HetCluster &v = recs[i];
        if (i == 0 || recs[i - 1].seq != v.seq || recs[i - 1].pos != v.pos) firsts = 0;
        const unsigned bit = 1u << het_cluster_base(v, 0);
        if (!(firsts & bit)) ++counts[4 * (size_t)v.seq + 1];
        firsts |= bit;
        ++counts[4 * (size_t)v.seq + 2];
    }
    return 0;
}

}  // namespace jk
