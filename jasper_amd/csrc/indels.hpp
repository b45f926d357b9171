// indels.hpp -- indel scan of a set of sequences against the resident read table (indels.hip).
//
// An extension, the length-changing half of the variant scan (variants.hpp): the candidates of its dense scan -- a window that ends at p
// whose k-mer with the last base replaced by x is solid -- are also the first k-mer of an insertion of x before p and of a deletion at p
// that x follows.  A second check kernel tests those hypotheses (semantics: include/jasper_hip.h, jasper_indel_scan); the substitution
// check runs over the same candidates afterwards, so one call answers both questions.
#pragma once
#include "variants.hpp"

namespace jk {

enum { IT_INS = 1, IT_DEL = 2 };
constexpr int INDEL_MAX_LEN = 16;

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

struct IndelOut {
    std::vector<uint64_t> counts;    // 4 per sequence: ins_het, ins_error, del_het, del_error
    std::vector<Indel> recs;         // ordered by (seq, pos, type, len, base)
    VariantOut var;                  // what variant_scan_device gives on the same input
    double seconds = 0;              // device time (HIP events) of the scan and all check kernels
    double check_seconds = 0;        // ... of indels_check_kernel alone
    uint64_t lookups = 0;            // table lookups indels_check_kernel made (its last run)
    int retried = 0;                 // the indel check was repeated with a larger record list
};

int indel_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int max_len, IndelOut &out, std::string &err);
int indel_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, IndelOut &out, std::string &err);

}  // namespace jk
