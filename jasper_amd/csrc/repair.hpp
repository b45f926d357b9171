// repair.hpp -- the repair stage: the scans' error records applied to the text on the GPU, in rounds (repair.hip).
//
// An extension, and the step after the scans: every error record of the variant, the indel (with its mixed half) and the compound scan
// says "the reads hold y where the sequence holds the R bytes from p on".  A round runs the two scans that carry all of them on the text in
// HBM, the host picks the edits that cannot disturb each other's evidence (repair_host.hpp), and one kernel writes the new text -- a
// gather-copy of the old one around the edits.  The text goes up once and comes down once (semantics: include/jasper_hip.h, jasper_repair).
#pragma once
#include "compound.hpp"
#include "indels.hpp"
#include "repair_host.hpp"

namespace jk {

constexpr int REPAIR_THREADS = 256, REPAIR_TILE = REPAIR_THREADS * 16;      // OUTPUT bytes per workgroup of repair_apply_kernel
constexpr int REPAIR_CHUNK = 256;                                           // edits it stages into LDS at a time

struct RepairRound {               // (layout of the public jasper_repair_round)
    uint64_t records, accepted, conflicts, ambiguous, unreliable_before, unreliable_after;
};

struct RepairOut {
    std::string text;                  // the final sequences back to back ...
    std::vector<int64_t> offsets;      // ... and their n_seqs + 1 boundaries
    std::vector<Edit> edits;           // every applied edit, ordered by (round, seq, pos); pos in the coordinates of that round's input
    std::vector<RepairRound> rounds;   // every round that scanned: the last one accepted nothing unless the loop ran out of rounds
    ReportOut before, after;           // what kmer_report_device gives on the input and on the final text
    double seconds = 0;                // device time (HIP events) of the scans and the apply kernel
    double apply_seconds = 0;          // ... of repair_apply_kernel alone
};

// sequence i = d_text[offsets[i] .. offsets[i+1]) on the table's device; offsets is a host array of n_seqs + 1 entries.  The input text
// is not written.
int repair_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, uint32_t thre, int indel_max_len, int compound_max_len, int rounds, RepairOut &out,
                  std::string &err);
int repair_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int indel_max_len, int compound_max_len, int rounds, RepairOut &out,
                std::string &err);
// The kernel alone on a caller's edit list (sorted by (seq, pos); check_edits says what else it has to be): out gets text and offsets.
// A list that is refused launches nothing.
int apply_edits_device(Table &T, int n_seqs, const uint8_t *d_text, const int64_t *offsets, const Edit *edits, uint64_t n_edits, RepairOut &out, std::string &err);
int apply_edits_host(Table &T, int n_seqs, const char *const *seqs, const int64_t *lens, const Edit *edits, uint64_t n_edits, RepairOut &out, std::string &err);

}  // namespace jk
