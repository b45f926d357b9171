// spectra.hpp -- copy-number k-mer spectrum: the join of two resident tables (reads R, assembly A) on the device (spectra.hip).
//
// An extension: the reference has no counterpart.  Semantics: include/jasper_hip.h (jasper_table_spectrum).
#pragma once
#include "table.hpp"
#include <string>

namespace jk {

constexpr int SP_ROWS = 6;          // copies in the assembly: 0, 1, 2, 3, 4, 5 and more
constexpr int SP_COLS = 10002;      // count in the reads, binned as the histogram is: 0 .. 10000, 10001 and more
constexpr int SP_LDS_COLS = 1024;   // columns below it are binned in LDS, the rare tail goes to the global matrix by atomics
constexpr int SP_THREADS = 256, SP_BATCH = 4;   // slots a thread has in flight per trip

// out: SP_ROWS * SP_COLS cells, row-major (host memory); seconds: device time (HIP events) of the sweeps
int table_spectrum(Table &R, Table &A, uint64_t *out, double *seconds, std::string &err);

}  // namespace jk
