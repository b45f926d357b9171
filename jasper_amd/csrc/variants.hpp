// variants.hpp -- variant scan of a set of sequences against the resident read table (variants.hip).
//
// An extension: the reference knows the situation (fixdiploid, fix_k_case_sub in src/jasper.py) but only acts on it inside its walk
// and reports nothing.  The dense scan of report.hip with three more probes per window -- the window's last base replaced by each of
// the other three -- and, for the few positions where one of them is solid, a check of all k windows that cover the position
// (semantics: include/jasper_hip.h, jasper_variant_scan).  The same candidates are the first k-mer of an insertion or a deletion at that
// position: indels.hpp tests those hypotheses.
#pragma once
#include "report.hpp"
#include <string>
#include <vector>

namespace jk {

enum { VK_REJECTED = 0, VK_HET = 1, VK_ERROR = 2 };   // kind of a record; 0 only on the device: a candidate the check dropped

// a substitution site (layout of the public jasper_variant)
struct Variant {
    int64_t pos;
    uint32_t seq;
    uint32_t ref_min;
    uint32_t alt_min;
    uint8_t ref, alt, kind, pad;      // ref / alt: 'A', 'C', 'G', 'T'
};
static_assert(sizeof(Variant) == 24, "layout of jasper_variant");

struct VariantOut {
    std::vector<uint64_t> counts;    // 3 per sequence: evaluated, het, error
    std::vector<Variant> recs;       // ordered by (seq, pos, alt)
    uint64_t candidates = 0;         // what the dense scan handed to the check
    double seconds = 0;              // device time (HIP events) of the kernels
    int retried = 0;                 // the scan was repeated with a larger candidate list
};

// sequence i = d_text[offsets[i] .. offsets[i+1]) on the table's device; offsets is a host array of n_seqs + 1 entries
int variant_scan_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, VariantOut &out, std::string &err);
int variant_scan_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, VariantOut &out, std::string &err);

// The two stages of variant_scan_device, for the indel scan (indels.hip), which puts its own check between them.  The caller has
// validated n_seqs / offsets / thre, selected the device, materialized the table and reset `out`.
struct VariantStage {
    uint64_t ntiles = 0, ncand = 0;
    int64_t *d_offs = nullptr;                  // the offsets on the device
    unsigned long long *d_cnt = nullptr;        // evaluated positions per sequence
    unsigned long long *d_ctl = nullptr;        // the variant kernels' control words
    Variant *d_cand = nullptr;                  // ncand candidates as variants_scan_kernel wrote them: alt = the alternative's CODE, kind 0
};
int variant_scan_stage(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, const char *what, VariantOut &out, VariantStage &S,
                       std::string &err);
int variant_check_stage(Table &T, int n_seqs, const uint8_t *d_text, uint32_t thre, const char *what, const VariantStage &S, VariantOut &out, std::string &err);

}  // namespace jk
