// select.hpp -- a set of k-mers defined by a join of up to three resident tables, MATERIALISED as a table of its own (select.hip):
// the keys of `src` with a count of at least thre_src that `absent` does not hold and (when `solid` is given) that `solid` holds at
// least thre_solid times, each with its count in src.
//
// An extension: the reference has no counterpart.  It is the hap-mer census (hapmers.hip) with the keys kept instead of counted:
// the census says how many such keys there are, this makes them the table the binning kernels (readbins.hip and what is built on
// it) probe.  Semantics: include/jasper_hip.h (jasper_table_select).
#pragma once
#include "table.hpp"
#include <string>

namespace jk {

constexpr uint64_t SEL_PIECE = 1ull << 24;     // slots of src per piece: the entry buffer holds one piece's slots (24 B each, 384 MiB at most)
enum { SEL_CANDIDATES = 0, SEL_IN_ABSENT = 1, SEL_NOT_SOLID = 2, SEL_SELECTED = 3, SEL_NCOUNT = 4 };

// dst: an open table without a key (it is filled through Table::import_entries, piece by piece).  solid may be null, and may be an
// attached owner-sharded table; the other three are whole tables.  out4 = candidates, in_absent, not_solid, selected (summed over
// the pieces); seconds = device time of the select kernels (HIP events), without the imports.
int table_select(Table &dst, Table &src, Table &absent, Table *solid, uint32_t thre_src, uint32_t thre_solid, uint64_t out4[4], double *seconds, std::string &err);

// The counting sibling: dst = src - minus, key by key and in full 64-bit counts -- the keys of `src` whose count exceeds their count in
// `minus` (0 for a key it lacks), each with the difference.  Counting is additive, so when `minus` counts a part of what `src` counts,
// dst counts the rest (triobin --write-jf: all reads - the other haplotype's bin = own bin + unknown).  Semantics: include/jasper_hip.h
// (jasper_table_subtract).
constexpr uint64_t SUB_PIECE = SEL_PIECE;      // slots of src per piece (JASPER_SUBTRACT_PIECE=<slots> for tests)
enum { SUB_SWEPT = 0, SUB_MATCHED = 1, SUB_DROPPED = 2, SUB_UNDERFLOW = 3, SUB_KEPT = 4, SUB_NCOUNT = 5 };
// dst: an open table without a key; all three are whole tables of one k on one device, of any sizes, narrow or wide; src and minus are
// only read.  out5 = swept (keys of src), matched (those minus holds), dropped (difference 0), underflow (minus holds more: the key is
// left out), kept; swept = dropped + underflow + kept.  dst's occurrence counter becomes the sum of the differences.  seconds = device time of the subtract kernels (HIP events), without the imports.
int table_subtract(Table &dst, Table &src, Table &minus, uint64_t out5[5], double *seconds, std::string &err);

}  // namespace jk
