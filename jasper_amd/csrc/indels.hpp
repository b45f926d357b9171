// indels.hpp -- indel scan of a set of sequences against the resident read table (indels.hip).
//
// An extension, the length-changing half of the variant scan (variants.hpp): the candidates of its dense scan -- a window that ends at p
// whose k-mer with the last base replaced by x is solid -- are also the first k-mer of an insertion of x before p and of a deletion at p
// that x follows.  A second check kernel tests those hypotheses (semantics: include/jasper_hip.h, jasper_indel_scan); the substitution
// check runs over the same candidates afterwards, so one call answers both questions.  With `mixed` a third kernel searches, per
// candidate, the insertions of mixed bases that start with x (jasper_indel_scan_mixed); without it nothing of that runs or is allocated.
// With `cluster_len` > 0 a fourth kernel searches, per candidate, the replacements of up to cluster_len bytes by up to cluster_len bases
// where both the sequence and the replacement are solid -- clusters of heterozygous differences less than k apart, which every
// single-edit check rejects (jasper_indel_scan_clusters); with 0 nothing of that runs or is allocated.
#pragma once
#include "hetcluster_host.hpp"
#include "variants.hpp"

namespace jk {

enum { IT_INS = 1, IT_DEL = 2 };
constexpr int INDEL_MAX_LEN = 16;
constexpr int INDEL_FRONT = 64;      // the mixed search keeps at most this many prefixes of one length (JASPER_INDEL_FRONT)

// an insertion or a deletion (layout of the public jasper_indel)
struct Indel {
    int64_t pos;
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint16_t len;
    uint8_t type, base, kind;      // type: IT_INS / IT_DEL; base: 'A', 'C', 'G', 'T'; kind: VK_HET / VK_ERROR
    uint8_t pad[7];
};
static_assert(sizeof(Indel) == 32, "layout of jasper_indel");

// an insertion of mixed bases (layout of the public jasper_mixed_ins)
struct MixedIns {
    int64_t pos;
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint32_t bases;                // base i of the inserted string in bits 2i, 2i + 1; 0 above 2 * len
    uint16_t len;
    uint8_t kind;                  // VK_HET / VK_ERROR
    uint8_t pad[5];
};
static_assert(sizeof(MixedIns) == 32, "layout of jasper_mixed_ins");

struct IndelOut {
    std::vector<uint64_t> counts;    // 4 per sequence: ins_het, ins_error, del_het, del_error
    std::vector<Indel> recs;         // ordered by (seq, pos, type, len, base)
    VariantOut var;                  // what variant_scan_device gives on the same input
    double seconds = 0;              // device time (HIP events) of the scan and all check kernels
    double check_seconds = 0;        // ... of indels_check_kernel alone
    uint64_t lookups = 0;            // table lookups indels_check_kernel made (its last run)
    int retried = 0;                 // the indel check was repeated with a larger record list
    // the mixed half: empty unless the scan was asked for it
    bool mixed = false;
    std::vector<uint64_t> mixed_counts;    // 3 per sequence: mixed_het, mixed_error, complex
    std::vector<MixedIns> mixed_recs;      // ordered by (seq, pos, len, the inserted string)
    double mixed_seconds = 0;              // device time of indels_mixed_kernel (part of `seconds`)
    uint64_t mixed_lookups = 0;            // table lookups it made (its last run)
    int mixed_retried = 0;                 // it was repeated with a larger record list
    // the het-cluster half: empty unless the scan was asked for it
    int cluster_len = 0;
    std::vector<uint64_t> cluster_counts;  // 4 per sequence: searched, sites, records, complex
    std::vector<HetCluster> cluster_recs;  // ordered by (seq, pos, ref_len, len, y)
    double cluster_seconds = 0;            // device time of het_cluster_kernel (part of `seconds`)
    uint64_t cluster_lookups = 0;          // table lookups it made (its last run)
    int cluster_retried = 0;               // it was repeated with a larger record list
};

int indel_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, bool mixed, int cluster_len, IndelOut &out,
                      std::string &err);
int indel_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, bool mixed, int cluster_len, IndelOut &out,
                    std::string &err);

}  // namespace jk
