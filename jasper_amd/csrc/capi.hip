// capi.hip -- extern "C" surface of libjasper_hip.so (declared in include/jasper_hip.h)
#include "../../include/jasper_hip.h"
#include "ingest.hpp"
#include "polish_host.hpp"
#include "table.hpp"
#include "pgunzip.hpp"
#include "inflate_gpu.hpp"
#include "asmio.hpp"
#include "report.hpp"
#include "spectra.hpp"
#include "copies.hpp"
#include "diploid.hpp"
#include "hapmers.hpp"
#include "select.hpp"
#include "bincount.hpp"
#include "readbins.hpp"
#include "readtext.hpp"
#include "readroute.hpp"
#include "deflate_gpu.hpp"
#include "readgz.hpp"
#include "variants.hpp"
#include "indels.hpp"
#include "compound.hpp"
#include "repair.hpp"
#include "dups.hpp"
#include "gaps.hpp"
#include <zlib.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace jk;

static thread_local std::string g_err;
std::string &jasper_err_ref() { return g_err; }

struct jasper_result;
struct jasper_table {
    Table t;
    jasper_result *pending = nullptr;   // result whose polished text still lies in this table's workspace
};

struct jasper_result {
    jasper_table *owner = nullptr;       // non-null while the text is on the device
    std::vector<const uint8_t *> d_seqs;
    std::vector<int64_t> d_lens;
    std::vector<std::string> seqs;
    std::vector<jasper_fixrec> recs;
    std::vector<std::string> aux;
    int64_t qv[4] = {0, 0, 0, 0};
    std::vector<int64_t> qv_chunk;
    uint64_t lookups = 0;
    double seconds = 0;
    uint64_t n_segments = 0, n_respeculated = 0;
    int retried = 0;                     // the batch was repeated with 8x the room because a bound was exceeded
};

static_assert(sizeof(jasper_fixrec) == sizeof(FixRec), "public and device record layouts must match");

struct jasper_copyrep {
    CopyOut r;
};
struct jasper_pairscan {
    PairOut r;
};
struct jasper_dupmap {
    DupOut r;
};
struct jasper_hapscan {
    HapOut r;
};
struct jasper_varscan {
    VariantOut r;
};
struct jasper_indelscan {
    IndelOut r;
    jasper_varscan var;                  // r.var moved here: what jasper_indelscan_variants hands out
};
struct jasper_report {
    ReportOut r;
};
struct jasper_compscan {
    CompoundOut r;
    jasper_report rep;                   // the report of the same call, written by the scan itself: what jasper_compscan_report hands out
};
struct jasper_gapscan {
    GapOut r;
    jasper_report rep;                   // the report of the same call (empty after jasper_gap_search): what jasper_gapscan_report hands out
};
struct jasper_repaired {
    RepairOut r;
    jasper_report before, after;         // r.before / r.after moved here: what jasper_repaired_before / _after hand out
};
static_assert(sizeof(jasper_kmer_run) == sizeof(KmerRun) && offsetof(jasper_kmer_run, n_absent) == offsetof(KmerRun, n_absent) &&
                  offsetof(jasper_kmer_run, seq) == offsetof(KmerRun, seq) && offsetof(jasper_kmer_run, min_count) == offsetof(KmerRun, min_count),
              "public and device run layouts must match");

// copy a device-resident result's text to the host (before its workspace is reused, or when the caller asks for it)
static int result_fetch(jasper_result *r) {
    if (!r->owner) return JASPER_OK;
    jasper_table *t = r->owner;
    Table &T = t->t;
    hipError_t e = hipSetDevice(T.device);
    for (size_t c = 0; c < r->d_seqs.size() && e == hipSuccess; ++c) {
        r->seqs[c].resize((size_t)r->d_lens[c]);
        if (r->d_lens[c]) e = hipMemcpyAsync(&r->seqs[c][0], r->d_seqs[c], (size_t)r->d_lens[c], hipMemcpyDeviceToHost, T.stream);
    }
    if (e == hipSuccess) e = jk_stream_wait(T.stream);
    if (t->pending == r) t->pending = nullptr;
    r->owner = nullptr;
    if (e != hipSuccess) { g_err = std::string("fetching polished text: ") + hipGetErrorString(e); return JASPER_ERR; }
    return JASPER_OK;
}

#define CHK(x)                                                        \
    do {                                                              \
        hipError_t e_ = (x);                                          \
        if (e_ != hipSuccess) {                                       \
            g_err = std::string(#x) + ": " + hipGetErrorString(e_);   \
            return JASPER_ERR;                                        \
        }                                                             \
    } while (0)

// ---- what the scans' entry points and accessors share ---------------------------------------------------------------------------------
static bool host_args(int n_seqs, const char *const *seqs, const int64_t *lens) { return n_seqs <= 0 || (seqs && lens); }

// One scan call: args_ok is the entry point's own check of its text arguments, tables whether every table it needs is there.  The result
// object is made, filled by fill(*r) (0 = done) and handed out, or deleted.
template <class Res, class Fill> static int scan_call(bool args_ok, bool tables, int n_seqs, Res **out, Fill &&fill) {
    if (!args_ok || !tables || !out || n_seqs < 0) { g_err = "bad argument"; return JASPER_ERR; }
    *out = nullptr;
    Res *r = new Res();
    if (fill(*r)) { delete r; return JASPER_ERR; }
    *out = r;
    return JASPER_OK;
}
// The N counters of sequence seq out of a vector of N per sequence (null: there is no result object).  A half of a scan that did not run
// left its vector empty: zeros for each of the n_seqs sequences.
template <int N> static int counts_out(const std::vector<uint64_t> *v, size_t n_seqs, int seq, uint64_t *out) {
    if (!v || !out || seq < 0 || (size_t)seq >= n_seqs) { g_err = "bad argument"; return JASPER_ERR; }
    for (int i = 0; i < N; ++i) out[i] = v->empty() ? 0 : (*v)[N * (size_t)seq + i];
    return JASPER_OK;
}
template <int N> static int counts_out(const std::vector<uint64_t> *v, int seq, uint64_t *out) { return counts_out<N>(v, v ? v->size() / N : 0, seq, out); }
template <class Rec, class Pub> static int records_out(const std::vector<Rec> *v, const Pub **out, uint64_t *n) {
    static_assert(sizeof(Rec) == sizeof(Pub), "public and device record layouts must match");
    if (!v || !out || !n) { g_err = "bad argument"; return JASPER_ERR; }
    *out = reinterpret_cast<const Pub *>(v->data());
    *n = v->size();
    return JASPER_OK;
}
static int word_out(const uint64_t *v, uint64_t *n) {
    if (!v || !n) { g_err = "bad argument"; return JASPER_ERR; }
    *n = *v;
    return JASPER_OK;
}

// A repair call: scan_call, and the two reports moved to where their accessors hand them out.
template <class Fill> static int repair_call(bool args_ok, jasper_table *t, int n_seqs, jasper_repaired **out, Fill &&fill) {
    return scan_call(args_ok, t, n_seqs, out, [&](jasper_repaired &r) {
        const int rc = fill(r.r);
        r.before.r = std::move(r.r.before);
        r.after.r = std::move(r.r.after);
        return rc;
    });
}

extern "C" {

const char *jasper_last_error(void) { return g_err.c_str(); }

int jasper_device_count(int *n) {
    CHK(hipGetDeviceCount(n));
    return JASPER_OK;
}

int jasper_request_cancel(int on) { jk::g_cancel.store(on ? 1 : 0); return JASPER_OK; }

int jasper_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
    size_t f = 0, t = 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) { g_err = std::string("hipMemGetInfo: ") + hipGetErrorString(e); return JASPER_ERR; }
    if (free_bytes) *free_bytes = (uint64_t)f;
    if (total_bytes) *total_bytes = (uint64_t)t;
    return JASPER_OK;
}

int jasper_table_create(int k, uint64_t min_slots, int device, jasper_table **out) {
    if (!out) { g_err = "null out"; return JASPER_ERR; }
    jasper_table *h = new jasper_table();
    int rc = h->t.init(k, min_slots, device, g_err);
    if (rc) { h->t.destroy(); delete h; return rc; }
    *out = h;
    return JASPER_OK;
}

int jasper_table_load_jf(const char *path, int device, jasper_table **out) {
    if (!out || !path) { g_err = "null argument"; return JASPER_ERR; }
    JfHeader h;
    int rc = jf_read_header(path, h, g_err);
    if (rc) return rc == -3 ? JASPER_ERR_FORMAT : JASPER_ERR;
    jasper_table *t = nullptr;
    rc = jasper_table_create(h.key_len / 2, std::max<uint64_t>(1u << 16, 2 * h.n_records), device, &t);
    if (rc) return rc;
    Table *T = &t->t;
    rc = T->load_jf_records(path, h.data_offset, h.n_records, h.key_len, h.counter_len, g_err);
    if (rc) { jasper_table_destroy(t); return rc < -1 ? rc : JASPER_ERR; }
    *out = t;
    return JASPER_OK;
}

int jasper_table_load_jf_part(const char *path, int device, uint32_t part, uint32_t nparts, jasper_table **out) {
    if (!out || !path || nparts == 0 || part >= nparts) { g_err = "bad argument"; return JASPER_ERR; }
    JfHeader h;
    int rc = jf_read_header(path, h, g_err);
    if (rc) return rc == -3 ? JASPER_ERR_FORMAT : JASPER_ERR;
    const uint64_t lo = h.n_records / nparts * part + std::min<uint64_t>(part, h.n_records % nparts);
    const uint64_t n = h.n_records / nparts + (part < h.n_records % nparts ? 1 : 0);
    const uint64_t rec = (uint64_t)((h.key_len + 7) / 8) + (uint64_t)h.counter_len;
    jasper_table *t = nullptr;
    rc = jasper_table_create(h.key_len / 2, std::max<uint64_t>(1u << 16, 2 * n), device, &t);
    if (rc) return rc;
    rc = t->t.load_jf_records(path, h.data_offset + lo * rec, n, h.key_len, h.counter_len, g_err);
    if (rc) { jasper_table_destroy(t); return rc < -1 ? rc : JASPER_ERR; }
    *out = t;
    return JASPER_OK;
}

int jasper_table_write_jf(jasper_table *t, const char *path, const char *const *cmdline, int n_cmdline) {
    if (!t || !path || n_cmdline < 0 || (n_cmdline && !cmdline)) { g_err = "null argument"; return JASPER_ERR; }
    return t->t.write_jf(path, cmdline, n_cmdline, g_err) ? JASPER_ERR : JASPER_OK;
}

int jasper_debug_mix(int k, int inverse, uint64_t hi, uint64_t lo, uint64_t out2[2]) {
    if (k < 1 || k > 64 || !out2) { g_err = "bad arguments"; return JASPER_ERR; }
    const u128 r = inverse ? unmix(mk(hi, lo), 2 * k) : mix(mk(hi, lo), 2 * k);
    out2[0] = r.hi;
    out2[1] = r.lo;
    return JASPER_OK;
}

void jasper_table_destroy(jasper_table *t) {
    if (!t) return;
    if (t->pending) (void)result_fetch(t->pending);   // a live result must not lose its text with the table
    t->t.destroy();
    delete t;
}

int jasper_table_info(jasper_table *t, int *k, uint64_t *slots, uint64_t *distinct, uint64_t *occurrences) {
    if (t->t.read_stats(g_err)) return JASPER_ERR;
    if (k) *k = t->t.k;
    if (slots) *slots = t->t.nslots;
    if (distinct) *distinct = t->t.h_stats[ST_DISTINCT];
    if (occurrences) *occurrences = t->t.h_stats[ST_OCCURRENCES];
    return JASPER_OK;
}

int jasper_table_sync(jasper_table *t) {
    CHK(hipSetDevice(t->t.device));
    CHK(jk_stream_wait(t->t.stream));
    return JASPER_OK;
}

int jasper_table_clear(jasper_table *t) { return t->t.clear(g_err) ? JASPER_ERR : JASPER_OK; }

int jasper_count_bases(jasper_table *t, const char *bases, uint64_t n) {
    t->t.reset_timing();
    return t->t.count_host(bases, n, g_err);
}

int jasper_count_bases_device(jasper_table *t, const void *d_bases, uint64_t n) {
    t->t.reset_timing();
    return t->t.count_device((const uint8_t *)d_bases, n, g_err);
}

int jasper_count_reads_text(jasper_table *t, const char *text, uint64_t n) {
    t->t.reset_timing();
    Table *T = &t->t;
    FastxParser p([T](const char *b, size_t m) { return T->count_host(b, m, g_err); });
    int rc = p.feed(text, n);
    if (!rc) rc = p.finish();
    if (rc && !p.error().empty()) g_err = p.error();
    return rc;
}

int jasper_count_reads_file_ranges(jasper_table *t, const char *const *paths, const int64_t *begins, const int64_t *ends, int n_paths) {
    if (!begins || !ends) { g_err = "null range arrays"; return JASPER_ERR; }
    t->t.reset_timing();
    Table *T = &t->t;
    T->ingest_gpu_bytes = T->ingest_host_bytes = 0;
    T->ingest_begin = begins;
    T->ingest_end = ends;
    const int rc = T->count_files_gpu(paths, n_paths, &T->ingest_gpu_bytes, &T->ingest_host_bytes, g_err);
    T->ingest_begin = T->ingest_end = nullptr;
    return rc < -1 ? rc : (rc ? JASPER_ERR : JASPER_OK);
}

int jasper_count_reads_files(jasper_table *t, const char *const *paths, int n_paths) {
    t->t.reset_timing();
    Table *T = &t->t;
    T->ingest_gpu_bytes = T->ingest_host_bytes = 0;
    for (uint64_t &v : T->inflate_stats) v = 0;
    if (!getenv("JASPER_INGEST_HOST")) {       // text parsed on the GPU; the host state machine takes over whatever is not plain 4-line FASTQ / FASTA
        const int rc = T->count_files_gpu(paths, n_paths, &T->ingest_gpu_bytes, &T->ingest_host_bytes, g_err);
        return rc < -1 ? rc : (rc ? JASPER_ERR : JASPER_OK);
    }
    FastxParser p([T](const char *b, size_t m) { return T->count_host(b, m, g_err); });
    std::string e;
    int rc = parse_files(paths, n_paths, p, e);
    if (rc && !e.empty()) g_err = e;
    return rc;
}

int jasper_last_ingest(jasper_table *t, uint64_t *gpu_bytes, uint64_t *host_bytes) {
    if (gpu_bytes) *gpu_bytes = t->t.ingest_gpu_bytes;
    if (host_bytes) *host_bytes = t->t.ingest_host_bytes;
    return JASPER_OK;
}

int jasper_last_inflate(jasper_table *t, uint64_t stats[6]) {
    if (!t || !stats) { g_err = "bad argument"; return JASPER_ERR; }
    for (int i = 0; i < GZS_N; ++i) stats[i] = t->t.inflate_stats[i];
    return JASPER_OK;
}

int jasper_last_count_timing(jasper_table *t, double *kernel_ms, uint64_t *launches) {
    if (kernel_ms) *kernel_ms = t->t.count_kernel_ms;
    if (launches) *launches = t->t.count_launches;
    return JASPER_OK;
}

int jasper_last_count_stages(jasper_table *t, double stage_ms[8], uint64_t *partitioned_launches, int *path) {
    for (int i = 0; i < 8; ++i) stage_ms[i] = t->t.part_stage_ms[i];
    if (partitioned_launches) *partitioned_launches = t->t.count_partitioned_launches;
    if (path) *path = t->t.count_path;
    return JASPER_OK;
}

int jasper_histogram_part(jasper_table *t, uint32_t part, uint32_t nparts, uint64_t *out10002) {
    if (nparts == 0 || part >= nparts || !out10002) { g_err = "bad partition"; return JASPER_ERR; }
    return t->t.histogram_part(part, nparts, out10002, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_histogram_is_fused(jasper_table *t) { return t && t->t.histo_cached ? 1 : 0; }

int jasper_histogram(jasper_table *t, uint64_t *out10002) { return t->t.histogram(out10002, g_err); }

int jasper_lookup(jasper_table *t, const char *chars, const int64_t *offsets, uint64_t n, uint32_t *out) {
    return t->t.lookup_strings(chars, offsets, n, out, g_err);
}

int jasper_table_export_device(jasper_table *t, uint64_t *n_entries, void **d_entries) {
    unsigned long long *p = nullptr;
    int rc = t->t.export_entries(n_entries, &p, g_err);
    if (rc) return rc;
    *d_entries = p;
    return JASPER_OK;
}

int jasper_table_export_to(jasper_table *t, void *d_dst, uint64_t cap_entries, uint64_t *n_entries) {
    unsigned long long *p = nullptr;
    uint64_t n = 0;
    int rc = t->t.export_entries(&n, &p, g_err);
    if (rc) return rc;
    if (n > cap_entries) { (void)hipFree(p); g_err = "export buffer too small"; return JASPER_ERR_CAPACITY; }
    if (n) CHK(hipMemcpy(d_dst, p, n * 24, hipMemcpyDeviceToDevice));
    CHK(hipFree(p));
    *n_entries = n;
    return JASPER_OK;
}

int jasper_table_import_device(jasper_table *t, const void *d_entries, uint64_t n_entries) {
    return t->t.import_entries((const unsigned long long *)d_entries, n_entries, g_err);
}

int jasper_table_export_packed(jasper_table *t, void *d_dst, uint64_t cap_entries, uint64_t *n_entries, uint32_t part, uint32_t nparts) {
    if (nparts == 0 || part >= nparts) { g_err = "bad partition"; return JASPER_ERR; }
    return t->t.export_packed(d_dst, cap_entries, n_entries, part, nparts, g_err);
}
int jasper_table_import_packed(jasper_table *t, const void *d_src, uint64_t n_entries, int mode) {
    return t->t.import_packed(d_src, n_entries, mode, g_err);
}
int jasper_table_import_packed_multi(jasper_table *t, const void *const *d_srcs, const uint64_t *counts, uint32_t n_src) {
    if (!d_srcs || !counts) { g_err = "null argument"; return JASPER_ERR; }
    return t->t.import_packed_multi(d_srcs, counts, n_src, g_err);
}
int jasper_table_reserve(jasper_table *t, uint64_t min_slots) { return t->t.reserve(min_slots, g_err); }

int jasper_table_fit(jasper_table *t, double max_load) { return t->t.fit(max_load, g_err); }
int jasper_table_export_owner(jasper_table *t, void *d_dst, uint64_t cap_entries, uint32_t n_owners, uint64_t *counts) {
    if (!counts) { g_err = "counts is null"; return JASPER_ERR; }
    return t->t.export_owner(d_dst, cap_entries, n_owners, 0, counts, g_err);
}
int jasper_read_feed_start(jasper_table *t, const char *const *paths, const int64_t *begins, const int64_t *ends, int n_paths) {
    if (!t || n_paths < 0 || (n_paths && !paths) || ((begins == nullptr) != (ends == nullptr))) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.feed_start(paths, begins, ends, n_paths, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_read_feed_next(jasper_table *t, const void **d_bases, uint64_t *n) {
    if (!t || !d_bases || !n) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.feed_next(d_bases, n, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_read_feed_release(jasper_table *t) {
    if (!t) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.feed_release(g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_count_exchange_plan(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, uint64_t *out8) {
    if (!t || !out8) { g_err = "bad argument"; return JASPER_ERR; }
    const int rc = t->t.xchg_plan(piece_max, records_max, n_owners, out8, g_err);
    return rc == 0 ? JASPER_OK : rc == 1 ? 1 : JASPER_ERR;
}
int jasper_count_exchange_scan(jasper_table *t, const void *d_bases, uint64_t n, uint64_t pos, uint64_t end, uint64_t piece_max, uint32_t n_owners, void *d_deferred,
                               uint64_t deferred_cap, uint64_t *records) {
    if (!t || !d_deferred || !records || (n && !d_bases)) { g_err = "bad argument"; return JASPER_ERR; }
    if (pos == 0) t->t.reset_timing();                       // (the first round of a call: stage times are per call, like the other count entry points)
    return t->t.xchg_scan((const uint8_t *)d_bases, n, pos, end, piece_max, n_owners, d_deferred, deferred_cap, records, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_count_exchange_partition(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, void *d_send, void *d_send_counts, void *d_deferred,
                                    uint64_t deferred_cap) {
    if (!t || !d_send || !d_send_counts || !d_deferred) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.xchg_partition(piece_max, records_max, n_owners, d_send, d_send_counts, d_deferred, deferred_cap, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_count_exchange_dedupe(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, void *d_send, void *d_send_counts, uint32_t *max_fill,
                                 int *count_bits) {
    if (!t || !d_send || !d_send_counts || !max_fill || !count_bits) { g_err = "bad argument"; return JASPER_ERR; }
    const int rc = t->t.xchg_dedupe(piece_max, records_max, n_owners, d_send, d_send_counts, max_fill, count_bits, g_err);
    return rc == 0 ? JASPER_OK : rc == 1 ? 1 : JASPER_ERR;
}
int jasper_count_exchange_insert(jasper_table *t, const void *d_recv, const void *d_recv_counts, uint64_t piece_max, uint64_t records_max, uint32_t n_owners,
                                 uint32_t self, const void *d_deferred_all, uint64_t n_deferred_all, int whole_input, uint32_t slice_cap, int count_bits) {
    if (!t || !d_recv || !d_recv_counts || self >= n_owners || (n_deferred_all && !d_deferred_all) || count_bits < 0) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.xchg_insert(d_recv, d_recv_counts, piece_max, records_max, n_owners, self, d_deferred_all, n_deferred_all, whole_input, slice_cap, count_bits, g_err)
               ? JASPER_ERR : JASPER_OK;
}
int jasper_table_export_file_ranges(jasper_table *t, void *d_dst, uint64_t cap_entries, uint32_t n_ranges, int size_log2, uint64_t *counts) {
    if (!counts || size_log2 < 1) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.export_owner(d_dst, cap_entries, n_ranges, size_log2, counts, g_err);
}
int jasper_table_write_jf_piece(jasper_table *t, const char *path, const char *const *cmdline, int n_cmdline, int size_log2, int what) {
    if (!t || !path || n_cmdline < 0 || (n_cmdline && !cmdline) || what < 0 || what > 2 || size_log2 < 1) { g_err = "bad argument"; return JASPER_ERR; }
    return t->t.write_jf(path, cmdline, n_cmdline, g_err, size_log2, what) ? JASPER_ERR : JASPER_OK;
}
int jasper_table_ipc_handle(jasper_table *t, void *out64) { return t->t.ipc_handle(out64, g_err) ? JASPER_ERR : JASPER_OK; }
int jasper_table_attach_ipc(jasper_table *t, const void *handles, uint32_t n, uint32_t self) {
    return t->t.attach_ipc(handles, n, self, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_table_attach_tables(jasper_table *t, jasper_table *const *shards, uint32_t n, uint32_t self) {
    if (n < 1 || n > MAX_SHARDS || !shards) { g_err = "attach: 1..8 shards"; return JASPER_ERR; }
    Table *p[MAX_SHARDS] = {};
    for (uint32_t i = 0; i < n; ++i) p[i] = shards[i] ? &shards[i]->t : nullptr;
    return t->t.attach_tables(p, n, self, g_err) ? JASPER_ERR : JASPER_OK;
}
// Can this process map these slot arrays at all?  Meant to be called from a THROW-AWAY process with a time limit: a mapping
// call that never returns (seen on this stack for one allocation size) then costs a killed helper, not a hung rank.
int jasper_table_release_retired(jasper_table *t) {
    if (!t) { g_err = "bad argument"; return JASPER_ERR; }
    t->t.release_retired();
    return JASPER_OK;
}

int jasper_inflate_file(const char *path, int threads, uint64_t chunk_bytes, const char *out_path, uint64_t *n_out, int *parallel) {
    if (!path) { g_err = "bad arguments"; return JASPER_ERR; }
    FILE *f = nullptr;
    if (out_path) { f = fopen(out_path, "wb"); if (!f) { g_err = std::string("cannot write ") + out_path; return JASPER_ERR; } }
    uint64_t total = 0;
    int par = 0, rc = JASPER_OK;
    size_t fsz = 0;
    { struct stat st; if (stat(path, &st) == 0) fsz = (size_t)st.st_size; }
    jk::ParallelGunzip pg(path, threads, chunk_bytes ? (size_t)chunk_bytes : jk::ParallelGunzip::chunk_for(fsz, threads));
    if (threads >= 2 && pg.open()) {
        par = 1;
        std::vector<std::vector<uint8_t>> pieces;
        while (pg.next(pieces))
            for (auto &pc : pieces) { total += pc.size(); if (f && !pc.empty() && fwrite(pc.data(), 1, pc.size(), f) != pc.size()) { g_err = "write error"; rc = JASPER_ERR; } }
        if (!pg.error().empty()) { g_err = pg.error(); rc = JASPER_ERR; }
    } else {
        gzFile g = gzopen(path, "rb");
        if (!g) { g_err = std::string("cannot open ") + path; rc = JASPER_ERR; }
        else {
            std::vector<char> buf(4u << 20);
            for (;;) {
                const int r = gzread(g, buf.data(), (unsigned)buf.size());
                if (r < 0) { g_err = std::string("read error in ") + path; rc = JASPER_ERR; break; }
                if (r == 0) break;
                total += (uint64_t)r;
                if (f && fwrite(buf.data(), 1, (size_t)r, f) != (size_t)r) { g_err = "write error"; rc = JASPER_ERR; break; }
            }
            gzclose(g);
        }
    }
    if (f) fclose(f);
    if (n_out) *n_out = total;
    if (parallel) *parallel = par;
    return rc;
}

int jasper_inflate_file_device(int device, const char *path, uint64_t chunk_bytes, const char *out_path, uint64_t *n_out, uint64_t stats[6]) {
    if (!path) { g_err = "bad arguments"; return JASPER_ERR; }
    uint64_t st[GZS_N] = {};
    uint64_t total = 0;
    int rc = JASPER_OK;
    FILE *f = nullptr;
    if (out_path) { f = fopen(out_path, "wb"); if (!f) { g_err = std::string("cannot write ") + out_path; return JASPER_ERR; } }
    hipStream_t s = nullptr;
    std::vector<void *> bufs;
    char *h_buf = nullptr;
    const size_t BUF = 64u << 20;
    GzdConfig cfg = GzdConfig::from_env();
    if (chunk_bytes) cfg.chunk = std::max<size_t>(4096, (size_t)chunk_bytes);
    cfg.slab = std::max(cfg.slab, 4 * cfg.chunk);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        if (f) fclose(f);
        g_err = "no device";
        return JASPER_ERR;
    }
    {
        DeviceGunzip dg(path, device, s, cfg, st);
        auto alloc = [&bufs](int, size_t bytes) -> void * {
            void *p = nullptr;
            if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            bufs.push_back(p);
            return p;
        };
        if (dg.open(alloc) && hipHostMalloc((void **)&h_buf, BUF, hipHostMallocDefault) == hipSuccess) {
            for (;;) {
                const long r = dg.read(h_buf, BUF);
                if (r < 0) { g_err = dg.err; rc = JASPER_ERR; break; }
                if (r == 0) break;
                total += (uint64_t)r;
                if (f && fwrite(h_buf, 1, (size_t)r, f) != (size_t)r) { g_err = "write error"; rc = JASPER_ERR; break; }
            }
        } else {
            // not for the device inflater (not a regular gzip file with a valid header, no device memory): zlib's reader, as
            // jasper_inflate_file reads such a file
            gzFile g = gzopen(path, "rb");
            if (!g) { g_err = std::string("cannot open ") + path; rc = JASPER_ERR; }
            else {
                std::vector<char> buf(4u << 20);
                for (;;) {
                    const int r = gzread(g, buf.data(), (unsigned)buf.size());
                    if (r < 0) { g_err = std::string("read error in ") + path; rc = JASPER_ERR; break; }
                    if (r == 0) break;
                    total += (uint64_t)r;
                    st[GZS_HOST_BYTES] += (uint64_t)r;
                    if (f && fwrite(buf.data(), 1, (size_t)r, f) != (size_t)r) { g_err = "write error"; rc = JASPER_ERR; break; }
                }
                gzclose(g);
            }
        }
    }
    (void)hipStreamSynchronize(s);
    for (void *p : bufs) (void)hipFree(p);
    if (h_buf) (void)hipHostFree(h_buf);
    (void)hipStreamDestroy(s);
    if (f) fclose(f);
    if (n_out) *n_out = total;
    if (stats) for (int i = 0; i < GZS_N; ++i) stats[i] = st[i];
    return rc;
}

int jasper_ipc_probe(int device, const void *handles, uint32_t n, uint32_t self) {
    if (!handles || n < 1 || n > MAX_SHARDS || self >= n) { g_err = "probe: 1..8 handles, self among them"; return JASPER_ERR; }
    CHK(hipSetDevice(device));
    for (uint32_t i = 0; i < n; ++i) {
        if (i == self) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, (const char *)handles + 64 * (size_t)i, 64);
        void *p = nullptr;
        CHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.device != device) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, device, at.device) != hipSuccess || !can) { (void)hipIpcCloseMemHandle(p); g_err = "no peer access"; return JASPER_ERR; }
        }
        CHK(hipIpcCloseMemHandle(p));
    }
    return JASPER_OK;
}

int jasper_table_detach(jasper_table *t) {
    if (hipSetDevice(t->t.device) != hipSuccess) { g_err = "hipSetDevice"; return JASPER_ERR; }
    (void)jk_stream_wait(t->t.stream);
    t->t.detach_shards();
    return JASPER_OK;
}
uint32_t jasper_owner_of(uint64_t hash_lo, uint64_t hash_hi, uint32_t n) { return owner_of(mk(hash_hi, hash_lo), n); }

int jasper_device_free(jasper_table *t, void *d_ptr) {
    CHK(hipSetDevice(t->t.device));
    CHK(hipFree(d_ptr));
    return JASPER_OK;
}

int jasper_table_export(jasper_table *t, uint64_t *n_entries, uint64_t *host_entries) {
    if (!host_entries) {
        if (t->t.read_stats(g_err)) return JASPER_ERR;
        *n_entries = t->t.h_stats[ST_DISTINCT];
        return JASPER_OK;
    }
    void *d = nullptr;
    uint64_t n = 0;
    int rc = jasper_table_export_device(t, &n, &d);
    if (rc) return rc;
    if (n > *n_entries) { (void)hipFree(d); g_err = "export buffer too small"; return JASPER_ERR_CAPACITY; }
    CHK(hipMemcpy(host_entries, d, n * 24, hipMemcpyDeviceToHost));
    CHK(hipFree(d));
    *n_entries = n;
    return JASPER_OK;
}

int jasper_table_import(jasper_table *t, const uint64_t *host_entries, uint64_t n_entries) {
    if (!n_entries) return JASPER_OK;
    CHK(hipSetDevice(t->t.device));
    void *d = nullptr;
    CHK(hipMalloc(&d, n_entries * 24));
    CHK(hipMemcpy(d, host_entries, n_entries * 24, hipMemcpyHostToDevice));
    int rc = t->t.import_entries((const unsigned long long *)d, n_entries, g_err);
    (void)hipFree(d);
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// polishing (host orchestration in polish_host.hip)
// ---------------------------------------------------------------------------------------------------
static int polish_common(jasper_table *t, int n_chunks, const char *const *seqs, const int64_t *lens, int solid_thre, int passes, int fix,
                         bool device_io, jasper_result **out, int keep = -1) {
    const bool device_in = device_io, keep_on_device = keep < 0 ? device_io : keep != 0;
    Table &T = t->t;
    if (T.k < 6) { g_err = "polishing needs k >= 6"; return JASPER_ERR; }
    if (passes < 0 || passes > 200) { g_err = "bad number of passes"; return JASPER_ERR; }
    if (solid_thre < 0) { g_err = "bad threshold"; return JASPER_ERR; }
    if (n_chunks < 0 || !out) { g_err = "bad arguments"; return JASPER_ERR; }
    if (t->pending && result_fetch(t->pending)) return JASPER_ERR;     // its text is about to be overwritten
    jasper_result *R = new jasper_result();
    *out = R;
    PolishOut po;
    int rc = run_polish(T, n_chunks, seqs, lens, solid_thre, passes, fix, po, g_err, device_in, keep_on_device, getenv("JASPER_POLISH_ROOMY") ? 1 : 0);      // (tests: the roomy sizes at once)
    if (rc == -2) {                      // a slack / record / scratch bound was too small for this input: once more with 8x the room
        R->retried = 1;
        po = PolishOut();
        rc = run_polish(T, n_chunks, seqs, lens, solid_thre, passes, fix, po, g_err, device_in, keep_on_device, 1);
    }
    R->seqs.swap(po.seqs);
    R->aux.swap(po.aux);
    R->recs.resize(po.recs.size());
    if (!po.recs.empty()) memcpy(R->recs.data(), po.recs.data(), po.recs.size() * sizeof(FixRec));
    for (int i = 0; i < 4; ++i) R->qv[i] = po.qv[i];
    R->qv_chunk.swap(po.qv_chunk);
    R->lookups = po.lookups;
    R->seconds = po.seconds;
    R->n_segments = po.n_segments;
    R->n_respeculated = po.n_respeculated;
    if (rc == 0 && keep_on_device) {
        R->d_seqs.swap(po.d_seqs);
        R->d_lens.swap(po.d_lens);
        R->owner = t;
        t->pending = R;
    }
    if (rc == -4) return JASPER_ERR_REFERENCE_EXIT;
    if (rc == -2) return JASPER_ERR_CAPACITY;
    return rc ? JASPER_ERR : JASPER_OK;
}

int jasper_polish_batch(jasper_table *t, int n_chunks, const char *const *seqs, const int64_t *lens, int solid_thre,
                        int passes, int fix, jasper_result **out) {
    return polish_common(t, n_chunks, seqs, lens, solid_thre, passes, fix, false, out);
}

int jasper_polish_batch_device(jasper_table *t, int n_chunks, const void *d_text, const int64_t *offsets, int solid_thre,
                               int passes, int fix, jasper_result **out) {
    if (n_chunks < 0 || (n_chunks && (!d_text || !offsets))) { g_err = "bad arguments"; return JASPER_ERR; }
    std::vector<const char *> ptrs((size_t)n_chunks);
    std::vector<int64_t> lens((size_t)n_chunks);
    for (int c = 0; c < n_chunks; ++c) {
        if (offsets[c + 1] < offsets[c]) { g_err = "offsets must not decrease"; return JASPER_ERR; }
        ptrs[c] = (const char *)d_text + offsets[c];
        lens[c] = offsets[c + 1] - offsets[c];
    }
    return polish_common(t, n_chunks, ptrs.data(), lens.data(), solid_thre, passes, fix, true, out);
}

// the chunk records of the listed batch files of a split assembly (asmio.cpp), straight from the job's arena; result chunk i is
// the i-th record of the files in list order
static int asm_records(const jasper_asm *a, const uint32_t *files, uint32_t n_files, std::vector<size_t> &recs) {
    if (!a || (n_files && !files)) { g_err = "bad arguments"; return JASPER_ERR; }
    for (uint32_t i = 0; i < n_files; ++i) {
        if ((size_t)files[i] + 1 >= a->file_first.size()) { g_err = "batch file out of range"; return JASPER_ERR; }
        for (size_t c = a->file_first[files[i]]; c < a->file_first[files[i] + 1]; ++c) recs.push_back(c);
    }
    return JASPER_OK;
}

int jasper_asm_polish(jasper_table *t, jasper_asm *a, const uint32_t *files, uint32_t n_files, int solid_thre, int passes, int fix, jasper_result **out) {
    std::vector<size_t> recs;
    if (int rc = asm_records(a, files, n_files, recs)) return rc;
    if (recs.size() > (size_t)INT32_MAX) { g_err = "too many chunk records for one call"; return JASPER_ERR; }
    std::vector<const char *> ptrs(recs.size());
    std::vector<int64_t> lens(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
        const AsmChunk &ch = a->chunks[recs[i]];
        ptrs[i] = (const char *)a->arena + a->contigs[ch.contig].seq_off + ch.ci;
        lens[i] = (int64_t)ch.len;
    }
    // host text in; the polished text stays in HBM until jasper_asm_take copies it -- into the job's pinned buffer when there is one
    return polish_common(t, (int)recs.size(), ptrs.data(), lens.data(), solid_thre, passes, fix, false, out, 1);
}

static void asm_gpu_release(jasper_asm *a) {
    if (a->arena_registered) { (void)hipHostUnregister(a->arena); a->arena_registered = false; }
    if (a->out_pinned) { (void)hipHostFree(a->out_pinned); a->out_pinned = nullptr; a->out_cap = 0; }
}

// (any thread, once: blocks while the GPU runtime starts -- the caller runs it beside the counting)
int jasper_asm_pin(jasper_asm *a, int device) {
    if (!a) { g_err = "bad arguments"; return JASPER_ERR; }
    CHK(hipSetDevice(device));
    a->gpu_release = asm_gpu_release;
    if (!a->arena_registered && a->arena && a->arena_cap)
        a->arena_registered = hipHostRegister(a->arena, a->arena_cap, hipHostRegisterDefault) == hipSuccess;      // (refused: the copies are staged, as before)
    (void)hipGetLastError();
    if (!a->out_pinned) {
        const size_t own = a->own_bases ? (size_t)a->own_bases : a->arena_len;      // (one GPU of several: its own batch files' records only)
        const size_t want = own + own / 64 + (1u << 20);
        if (hipHostMalloc((void **)&a->out_pinned, want, hipHostMallocDefault) == hipSuccess) a->out_cap = want;
        else { a->out_pinned = nullptr; (void)hipGetLastError(); }
    }
    return JASPER_OK;
}

int jasper_asm_take(jasper_asm *a, jasper_result *r, const uint32_t *files, uint32_t n_files) {
    std::vector<size_t> recs;
    if (int rc = asm_records(a, files, n_files, recs)) return rc;
    if (!r || r->seqs.size() != recs.size()) { g_err = "the result is not the one of these batch files"; return JASPER_ERR; }
    if (r->owner) {
        // still on the device: one copy per record into the job's pinned buffer (after what earlier calls put there); a buffer
        // that is missing or too small -> through the result's own host strings
        size_t total = 0;
        for (size_t i = 0; i < recs.size(); ++i) total += (size_t)r->d_lens[i];
        if (a->out_pinned && a->out_used + total <= a->out_cap) {
            Table &T = r->owner->t;
            CHK(hipSetDevice(T.device));
            size_t at = a->out_used;
            for (size_t i = 0; i < recs.size(); ++i) {
                const size_t n = (size_t)r->d_lens[i];
                if (n) CHK(hipMemcpyAsync(a->out_pinned + at, r->d_seqs[i], n, hipMemcpyDeviceToHost, T.stream));
                jasper_asm::Polished &P = a->polished[recs[i]];
                P.p = a->out_pinned + at;
                P.n = n;
                P.own.clear();
                at += n;
            }
            CHK(jk_stream_wait(T.stream));
            a->out_used = at;
            for (size_t i = 0; i < recs.size(); ++i) a->have[recs[i]] = 1;
            if (r->owner->pending == r) r->owner->pending = nullptr;
            r->owner = nullptr;              // (the text has left the device with the job: the result keeps records, counters, aux)
            return JASPER_OK;
        }
        if (result_fetch(r)) return JASPER_ERR;
    }
    for (size_t i = 0; i < recs.size(); ++i) {
        a->polished[recs[i]].p = nullptr;
        a->polished[recs[i]].own.swap(r->seqs[i]);
        a->have[recs[i]] = 1;
    }
    return JASPER_OK;
}

int jasper_result_num_chunks(const jasper_result *r) { return (int)r->seqs.size(); }
int jasper_result_seq(const jasper_result *r, int chunk, const char **seq, int64_t *len) {
    if (chunk < 0 || chunk >= (int)r->seqs.size()) { g_err = "chunk out of range"; return JASPER_ERR; }
    if (r->owner && result_fetch(const_cast<jasper_result *>(r))) return JASPER_ERR;
    *seq = r->seqs[chunk].data();
    *len = (int64_t)r->seqs[chunk].size();
    return JASPER_OK;
}
int jasper_result_seq_len(const jasper_result *r, int chunk, int64_t *len) {
    if (chunk < 0 || chunk >= (int)r->seqs.size()) { g_err = "chunk out of range"; return JASPER_ERR; }
    *len = r->owner ? r->d_lens[chunk] : (int64_t)r->seqs[chunk].size();
    return JASPER_OK;
}
int jasper_result_seq_device(const jasper_result *r, int chunk, const void **d_seq, int64_t *len) {
    if (chunk < 0 || chunk >= (int)r->seqs.size()) { g_err = "chunk out of range"; return JASPER_ERR; }
    if (!r->owner) { g_err = "the polished text of this result is no longer on the device"; return JASPER_ERR; }
    *d_seq = r->d_seqs[chunk];
    *len = r->d_lens[chunk];
    return JASPER_OK;
}
int jasper_result_records(const jasper_result *r, const jasper_fixrec **recs, uint64_t *n) {
    *recs = r->recs.data();
    *n = r->recs.size();
    return JASPER_OK;
}
int jasper_result_aux(const jasper_result *r, int chunk, const char **aux, uint64_t *n) {
    if (chunk < 0 || chunk >= (int)r->aux.size()) { g_err = "chunk out of range"; return JASPER_ERR; }
    *aux = r->aux[chunk].data();
    *n = r->aux[chunk].size();
    return JASPER_OK;
}
int jasper_result_qv(const jasper_result *r, int64_t out4[4]) {
    for (int i = 0; i < 4; ++i) out4[i] = r->qv[i];
    return JASPER_OK;
}
int jasper_result_lookups(const jasper_result *r, uint64_t *n) { *n = r->lookups; return JASPER_OK; }
double jasper_result_seconds(const jasper_result *r) { return r->seconds; }
int jasper_result_segments(const jasper_result *r, uint64_t *n_segments, uint64_t *n_respeculated) {
    if (n_segments) *n_segments = r->n_segments;
    if (n_respeculated) *n_respeculated = r->n_respeculated;
    return JASPER_OK;
}
int jasper_result_qv_chunk(const jasper_result *r, int chunk, int64_t out4[4]) {
    if (chunk < 0 || (size_t)(4 * chunk + 3) >= r->qv_chunk.size()) { g_err = "chunk out of range"; return JASPER_ERR; }
    for (int i = 0; i < 4; ++i) out4[i] = r->qv_chunk[4 * (size_t)chunk + i];
    return JASPER_OK;
}
int jasper_polish_cut_geometry(int k, int64_t out5[5]) {
    if (k < 1 || k > 64 || !out5) { g_err = "jasper_polish_cut_geometry: k must be 1 .. 64"; return JASPER_ERR; }
    const CutGeometry g = cut_geometry(k);
    out5[0] = g.tmin; out5[1] = g.cmin; out5[2] = g.clean_cell; out5[3] = g.w; out5[4] = g.m;
    return JASPER_OK;
}
int jasper_result_retried(const jasper_result *r) { return r ? r->retried : 0; }
void jasper_result_free(jasper_result *r) {
    if (r && r->owner && r->owner->pending == r) r->owner->pending = nullptr;
    delete r;
}

// ---- dense k-mer report (report.hip) ----
int jasper_kmer_report(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_report **out) {
    return scan_call(host_args(n_seqs, seqs, lens), t, n_seqs, out, [&](jasper_report &r) { return kmer_report_host(t->t, n_seqs, seqs, lens, thre, r.r, g_err); });
}
int jasper_kmer_report_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, jasper_report **out) {
    return scan_call(offsets, t, n_seqs, out, [&](jasper_report &r) { return kmer_report_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, r.r, g_err); });
}
int jasper_report_tile_windows(void) { return RP_TILE; }
int jasper_report_num_seqs(const jasper_report *r) { return r ? (int)(r->r.counts.size() / 4) : 0; }
int jasper_report_counts(const jasper_report *r, int seq, uint64_t out4[4]) { return counts_out<4>(r ? &r->r.counts : nullptr, seq, out4); }
int jasper_report_runs(const jasper_report *r, const jasper_kmer_run **runs, uint64_t *n) { return records_out(r ? &r->r.runs : nullptr, runs, n); }
double jasper_report_seconds(const jasper_report *r) { return r ? r->r.seconds : 0.0; }
int jasper_report_retried(const jasper_report *r) { return r ? r->r.retried : 0; }
void jasper_report_free(jasper_report *r) { delete r; }

// ---- copy-number k-mer spectrum (spectra.hip) ----
int jasper_spectrum_rows(void) { return SP_ROWS; }
int jasper_table_spectrum(jasper_table *reads, jasper_table *assembly, uint64_t *out_cells, double *device_seconds) {
    if (!reads || !assembly || !out_cells) { g_err = "bad argument"; return JASPER_ERR; }
    return table_spectrum(reads->t, assembly->t, out_cells, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}

// ---- copy-number scan (copies.hip) ----
int jasper_copy_report(jasper_table *reads, jasper_table *assembly, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak,
                       jasper_copyrep **out) {
    return scan_call(host_args(n_seqs, seqs, lens), reads && assembly, n_seqs, out,
                     [&](jasper_copyrep &r) { return copies_report_host(reads->t, assembly->t, n_seqs, seqs, lens, thre, peak, r.r, g_err); });
}
int jasper_copy_report_device(jasper_table *reads, jasper_table *assembly, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak,
                              jasper_copyrep **out) {
    return scan_call(offsets, reads && assembly, n_seqs, out,
                     [&](jasper_copyrep &r) { return copies_report_device(reads->t, assembly->t, n_seqs, (const uint8_t *)d_text, offsets, thre, peak, r.r, g_err); });
}
int jasper_copyrep_num_seqs(const jasper_copyrep *r) { return r ? (int)(r->r.counts.size() / 6) : 0; }
int jasper_copyrep_counts(const jasper_copyrep *r, int seq, uint64_t out6[6]) { return counts_out<6>(r ? &r->r.counts : nullptr, seq, out6); }
int jasper_copyrep_runs(const jasper_copyrep *r, const jasper_copy_run **runs, uint64_t *n) { return records_out(r ? &r->r.runs : nullptr, runs, n); }
double jasper_copyrep_seconds(const jasper_copyrep *r) { return r ? r->r.seconds : 0.0; }
int jasper_copyrep_retried(const jasper_copyrep *r) { return r ? r->r.retried : 0; }
void jasper_copyrep_free(jasper_copyrep *r) { delete r; }

// ---- pair spectrum and pair scan of a diploid assembly (diploid.hip) ----
static_assert(offsetof(jasper_pair_run, sum_reads) == offsetof(PairRun, sum_reads) && offsetof(jasper_pair_run, seq) == offsetof(PairRun, seq) &&
                  offsetof(jasper_pair_run, kind) == offsetof(PairRun, kind),
              "public and device run layouts must match");
int jasper_table_spectrum_pair(jasper_table *reads, jasper_table *assembly, jasper_table *alt, uint64_t *out_cells, double *device_seconds) {
    if (!reads || !assembly || !alt || !out_cells) { g_err = "bad argument"; return JASPER_ERR; }
    return table_spectrum_pair(reads->t, assembly->t, alt->t, out_cells, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_pair_scan(jasper_table *reads, jasper_table *other, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_pairscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), reads && other, n_seqs, out,
                     [&](jasper_pairscan &r) { return pair_scan_host(reads->t, other->t, n_seqs, seqs, lens, thre, r.r, g_err); });
}
int jasper_pairscan_num_seqs(const jasper_pairscan *r) { return r ? (int)(r->r.counts.size() / 6) : 0; }
int jasper_pairscan_counts(const jasper_pairscan *r, int seq, uint64_t out6[6]) { return counts_out<6>(r ? &r->r.counts : nullptr, seq, out6); }
int jasper_pairscan_runs(const jasper_pairscan *r, const jasper_pair_run **runs, uint64_t *n) { return records_out(r ? &r->r.runs : nullptr, runs, n); }
double jasper_pairscan_seconds(const jasper_pairscan *r) { return r ? r->r.seconds : 0.0; }
int jasper_pairscan_retried(const jasper_pairscan *r) { return r ? r->r.retried : 0; }
void jasper_pairscan_free(jasper_pairscan *r) { delete r; }

// ---- duplication map (dups.hip) ----
static_assert(offsetof(jasper_dup_run, mate_start) == offsetof(DupRun, mate_start) && offsetof(jasper_dup_run, n_deficit) == offsetof(DupRun, n_deficit) &&
                  offsetof(jasper_dup_run, mate_seq) == offsetof(DupRun, mate_seq) && offsetof(jasper_dup_run, strand) == offsetof(DupRun, strand),
              "jasper_dup_run is DupRun");
int jasper_dup_map(jasper_table *reads, jasper_table *assembly, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak,
                   jasper_dupmap **out) {
    return scan_call(host_args(n_seqs, seqs, lens), reads && assembly, n_seqs, out,
                     [&](jasper_dupmap &r) { return dup_map_host(reads->t, assembly->t, n_seqs, seqs, lens, thre, peak, r.r, g_err); });
}
int jasper_dup_map_device(jasper_table *reads, jasper_table *assembly, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak,
                          jasper_dupmap **out) {
    return scan_call(offsets, reads && assembly, n_seqs, out,
                     [&](jasper_dupmap &r) { return dup_map_device(reads->t, assembly->t, n_seqs, (const uint8_t *)d_text, offsets, thre, peak, r.r, g_err); });
}
int jasper_dupmap_num_seqs(const jasper_dupmap *r) { return r ? (int)(r->r.counts.size() / 7) : 0; }
int jasper_dupmap_counts(const jasper_dupmap *r, int seq, uint64_t out7[7]) { return counts_out<7>(r ? &r->r.counts : nullptr, seq, out7); }
int jasper_dupmap_runs(const jasper_dupmap *r, const jasper_dup_run **runs, uint64_t *n) { return records_out(r ? &r->r.runs : nullptr, runs, n); }
int jasper_dupmap_seconds(const jasper_dupmap *r, double *index, double *scan) {
    if (!r) { g_err = "bad argument"; return JASPER_ERR; }
    if (index) *index = r->r.index_seconds;
    if (scan) *scan = r->r.seconds;
    return JASPER_OK;
}
int jasper_dupmap_retried(const jasper_dupmap *r) { return r ? r->r.retried : 0; }
void jasper_dupmap_free(jasper_dupmap *r) { delete r; }

// ---- trio hap-mer scan and census (hapmers.hip) ----
int jasper_hapmer_scan(jasper_table *mat, jasper_table *pat, jasper_table *child, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre_mat,
                       uint32_t thre_pat, uint32_t thre_child, jasper_hapscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), mat && pat, n_seqs, out, [&](jasper_hapscan &r) {
        return hapmer_scan_host(mat->t, pat->t, child ? &child->t : nullptr, n_seqs, seqs, lens, thre_mat, thre_pat, thre_child, r.r, g_err);
    });
}
int jasper_hapmer_scan_device(jasper_table *mat, jasper_table *pat, jasper_table *child, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre_mat,
                              uint32_t thre_pat, uint32_t thre_child, jasper_hapscan **out) {
    return scan_call(offsets, mat && pat, n_seqs, out, [&](jasper_hapscan &r) {
        return hapmer_scan_device(mat->t, pat->t, child ? &child->t : nullptr, n_seqs, (const uint8_t *)d_text, offsets, thre_mat, thre_pat, thre_child, r.r, g_err);
    });
}
int jasper_hapscan_num_seqs(const jasper_hapscan *r) { return r ? (int)(r->r.counts.size() / 4) : 0; }
int jasper_hapscan_counts(const jasper_hapscan *r, int seq, uint64_t out4[4]) { return counts_out<4>(r ? &r->r.counts : nullptr, seq, out4); }
int jasper_hapscan_runs(const jasper_hapscan *r, const jasper_hap_run **runs, uint64_t *n) { return records_out(r ? &r->r.runs : nullptr, runs, n); }
double jasper_hapscan_seconds(const jasper_hapscan *r) { return r ? r->r.seconds : 0.0; }
int jasper_hapscan_retried(const jasper_hapscan *r) { return r ? r->r.retried : 0; }
void jasper_hapscan_free(jasper_hapscan *r) { delete r; }
int jasper_hapmer_census(jasper_table *mat, jasper_table *pat, jasper_table *child, jasper_table *assembly, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                         uint64_t out6[6], double *device_seconds) {
    if (!mat || !pat || !out6) { g_err = "bad argument"; return JASPER_ERR; }
    return hapmer_census(mat->t, pat->t, child ? &child->t : nullptr, assembly ? &assembly->t : nullptr, thre_mat, thre_pat, thre_child, out6, device_seconds, g_err)
               ? JASPER_ERR
               : JASPER_OK;
}

// ---- a join of tables as a table (select.hip) ----
int jasper_table_select(jasper_table *dst, jasper_table *src, jasper_table *absent, jasper_table *solid, uint32_t thre_src, uint32_t thre_solid, uint64_t out4[4],
                        double *device_seconds) {
    if (!dst || !src || !absent || !out4) { g_err = "bad argument"; return JASPER_ERR; }
    const int rc = table_select(dst->t, src->t, absent->t, solid ? &solid->t : nullptr, thre_src, thre_solid, out4, device_seconds, g_err);
    return rc == 0 ? JASPER_OK : rc == -2 ? JASPER_ERR_CAPACITY : JASPER_ERR;
}

int jasper_table_subtract(jasper_table *dst, jasper_table *src, jasper_table *minus, uint64_t out5[5], double *device_seconds) {
    if (!dst || !src || !minus || !out5) { g_err = "bad argument"; return JASPER_ERR; }
    const int rc = table_subtract(dst->t, src->t, minus->t, out5, device_seconds, g_err);
    return rc == 0 ? JASPER_OK : rc == -2 ? JASPER_ERR_CAPACITY : JASPER_ERR;
}

// ---- trio read binning (readbins.hip) ----
int jasper_read_bins(jasper_table *mat, jasper_table *pat, int64_t n_reads, const char *text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat, uint32_t *out_mat,
                     uint32_t *out_pat, double *device_seconds) {
    if (!mat || !pat) { g_err = "bad argument"; return JASPER_ERR; }
    return read_bins_host(mat->t, pat->t, n_reads, text, offsets, thre_mat, thre_pat, out_mat, out_pat, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_read_bins_device(jasper_table *mat, jasper_table *pat, int64_t n_reads, const void *d_text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat,
                            uint32_t *out_mat, uint32_t *out_pat, double *device_seconds) {
    if (!mat || !pat) { g_err = "bad argument"; return JASPER_ERR; }
    return read_bins_device(mat->t, pat->t, n_reads, (const uint8_t *)d_text, offsets, thre_mat, thre_pat, out_mat, out_pat, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
// ... from raw FASTQ / FASTA text (readtext.hip)
int jasper_read_text_bins(jasper_table *mat, jasper_table *pat, const char *text, int64_t n, int eof, int format, uint32_t thre_mat, uint32_t thre_pat, int64_t *used,
                          int64_t *n_records, int *status, int64_t *bad_record, double *device_seconds) {
    if (!mat || !pat) { g_err = "bad argument"; return JASPER_ERR; }
    return read_text_bins(mat->t, pat->t, text, n, eof, format, thre_mat, thre_pat, used, n_records, status, bad_record, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_read_text_fetch(jasper_table *mat, int64_t n_records, int64_t *rec_start, int64_t *head_end, int64_t *lens, uint32_t *out_mat, uint32_t *out_pat, uint8_t *out_seq) {
    if (!mat) { g_err = "bad argument"; return JASPER_ERR; }
    return read_text_fetch(mat->t, n_records, rec_start, head_end, lens, out_mat, out_pat, out_seq, g_err) ? JASPER_ERR : JASPER_OK;
}
// ... and the reads of chosen bins counted into tables of their own (bincount.hip)
namespace {
// the handles of a call's sinks as tables: false for a count outside 1 .. 3 or a null handle
bool sink_tables(int n_sinks, jasper_table *const *sinks, const uint32_t *masks, uint64_t *out, double *seconds, Table *tables[BC_SINKS], BinSinks &S) {
    if (n_sinks < 1 || n_sinks > BC_SINKS || !sinks || !masks || !out) { g_err = "count binned: bad arguments (1 to 3 sinks)"; return false; }
    for (int i = 0; i < n_sinks; ++i) {
        if (!sinks[i]) { g_err = "count binned: bad arguments (a sink without a table)"; return false; }
        tables[i] = &sinks[i]->t;
    }
    S = BinSinks{n_sinks, tables, masks, out, seconds};
    return true;
}
int binned_rc(int rc) { return rc == 0 ? JASPER_OK : rc == -2 ? JASPER_ERR_CAPACITY : JASPER_ERR; }
}  // namespace
int jasper_count_binned(int n_sinks, jasper_table *const *sinks, const uint32_t *masks, int64_t n_reads, const char *text, const int64_t *offsets, const uint8_t *codes,
                        uint64_t *out, double *seconds) {
    Table *tables[BC_SINKS];
    BinSinks S;
    if (!sink_tables(n_sinks, sinks, masks, out, seconds, tables, S)) return JASPER_ERR;
    return binned_rc(count_binned_host(S, n_reads, text, offsets, codes, g_err));
}
int jasper_count_binned_device(int n_sinks, jasper_table *const *sinks, const uint32_t *masks, int64_t n_reads, const void *d_text, const int64_t *offsets, const uint8_t *codes,
                               uint64_t *out, double *seconds) {
    Table *tables[BC_SINKS];
    BinSinks S;
    if (!sink_tables(n_sinks, sinks, masks, out, seconds, tables, S)) return JASPER_ERR;
    return binned_rc(count_binned_device(S, n_reads, (const uint8_t *)d_text, offsets, codes, nullptr, 0, g_err));
}
int jasper_read_text_count(jasper_table *mat, jasper_table *pat, int64_t n_records, const uint8_t *codes, int n_sinks, jasper_table *const *sinks, const uint32_t *masks,
                           uint64_t *out, double *seconds) {
    if (!mat) { g_err = "bad argument"; return JASPER_ERR; }
    Table *tables[BC_SINKS];
    BinSinks S;
    if (!sink_tables(n_sinks, sinks, masks, out, seconds, tables, S)) return JASPER_ERR;
    return binned_rc(read_text_count(mat->t, pat ? &pat->t : nullptr, n_records, codes, S, g_err));
}
// ... from a .gz file inflated on the device (readgz.hip), and the second pass's routing (readroute.hip)
struct jasper_gz_text {
    GzText *g = nullptr;
};
int jasper_gz_text_open(jasper_table *mat, const char *path, jasper_gz_text **out) {
    if (!mat || !path || !out) { g_err = "bad argument"; return JASPER_ERR; }
    *out = nullptr;
    GzText *g = gz_text_open(mat->t, path, g_err);
    if (!g) return JASPER_ERR;
    *out = new jasper_gz_text;
    (*out)->g = g;
    return JASPER_OK;
}
void jasper_gz_text_close(jasper_gz_text *h) {
    if (!h) return;
    delete h->g;
    delete h;
}
int jasper_gz_text_bins(jasper_gz_text *h, jasper_table *mat, jasper_table *pat, int64_t want, int *format, uint32_t thre_mat, uint32_t thre_pat, int64_t *n, int *eof,
                        int64_t *used, int64_t *n_records, int *status, int64_t *bad_record, double *device_seconds) {
    if (!h || !mat || !pat) { g_err = "bad argument"; return JASPER_ERR; }
    return gz_text_bins(*h->g, mat->t, pat->t, want, format, thre_mat, thre_pat, n, eof, used, n_records, status, bad_record, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_gz_text_copy(jasper_gz_text *h, int64_t from, int64_t len, uint8_t *dst) {
    if (!h) { g_err = "bad argument"; return JASPER_ERR; }
    return gz_text_copy(*h->g, from, len, dst, g_err) ? JASPER_ERR : JASPER_OK;
}
int jasper_gz_text_stats(jasper_gz_text *h, uint64_t stats[6]) {
    if (!h || !stats) { g_err = "bad argument"; return JASPER_ERR; }
    for (int i = 0; i < GZS_N; ++i) stats[i] = h->g->stats[i];
    return JASPER_OK;
}
// The four routing calls fill RouteJob / RouteOut and give RouteSeconds its places in device_seconds: the one place where a position in
// that array has a meaning (include/jasper_hip.h).  The two host-text calls read the array first, since a refusal of the arguments leaves
// the caller's numbers as they were; a session's route zeroes them before anything else.
int jasper_route_text(jasper_table *t, const uint8_t *text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *out0,
                      uint8_t *out1, uint8_t *out2, int64_t out_bytes[3], int64_t *mismatches, double *device_seconds) {
    if (!t) { g_err = "bad argument"; return JASPER_ERR; }
    uint8_t *const out[3] = {out0, out1, out2};
    double *const ds = device_seconds;
    RouteSeconds S = {ds ? ds[0] : 0, 0, 0};
    const int rc = route_text(t->t, text, false, n, RouteJob{n_seg, bounds, bins, first, check_from}, RouteOut{out, nullptr, out_bytes, nullptr, mismatches, nullptr}, S, g_err);
    if (ds) ds[0] = S.route;
    return rc ? JASPER_ERR : JASPER_OK;
}
int jasper_gz_text_route(jasper_gz_text *h, jasper_table *t, int64_t want, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *out0,
                         uint8_t *out1, uint8_t *out2, int64_t out_bytes[3], int64_t *got, int64_t *mismatches, double *device_seconds) {
    if (!h || !t) { g_err = "bad argument"; return JASPER_ERR; }
    uint8_t *const out[3] = {out0, out1, out2};
    double *const ds = device_seconds;
    RouteSeconds S = {0, 0, 0};
    const int rc = gz_text_route(*h->g, t->t, want, RouteJob{n_seg, bounds, bins, first, check_from}, RouteOut{out, nullptr, out_bytes, nullptr, mismatches, nullptr}, got, S, g_err);
    if (ds) { ds[0] = S.route; ds[1] = S.pull; }
    return rc ? JASPER_ERR : JASPER_OK;
}
// ... and the compressor (deflate_gpu.hip): a text as BGZF members, and the two routing calls with the three outputs compressed
int64_t jasper_deflate_bound(int64_t n) { return n < 0 ? -1 : (int64_t)deflate_bound((uint64_t)n); }
int jasper_deflate_bgzf(jasper_table *t, const uint8_t *text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_bytes, uint64_t counters[6], double *device_seconds) {
    if (!t) { g_err = "bad argument"; return JASPER_ERR; }
    return deflate_host(t->t, text, n, out, out_cap, out_bytes, counters, device_seconds, g_err) ? JASPER_ERR : JASPER_OK;
}
// (a null out_cap is refused here, in the words the call had for it: to route_text and gz_text_route it means plain outputs)
int jasper_route_text_gz(jasper_table *t, const uint8_t *text, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *out0,
                         uint8_t *out1, uint8_t *out2, const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *mismatches, uint64_t counters[6],
                         double *device_seconds) {
    if (!t) { g_err = "bad argument"; return JASPER_ERR; }
    if (!out_cap) { g_err = "route text: bad arguments"; return JASPER_ERR; }
    uint8_t *const out[3] = {out0, out1, out2};
    double *const ds = device_seconds;
    RouteSeconds S = {ds ? ds[0] : 0, 0, ds ? ds[1] : 0};
    const int rc = route_text(t->t, text, false, n, RouteJob{n_seg, bounds, bins, first, check_from}, RouteOut{out, out_cap, out_bytes, raw_bytes, mismatches, counters}, S, g_err);
    if (ds) { ds[0] = S.route; ds[1] = S.deflate; }
    return rc ? JASPER_ERR : JASPER_OK;
}
int jasper_gz_text_route_gz(jasper_gz_text *h, jasper_table *t, int64_t want, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from, uint8_t *out0,
                            uint8_t *out1, uint8_t *out2, const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *got, int64_t *mismatches,
                            uint64_t counters[6], double *device_seconds) {
    if (!h || !t) { g_err = "bad argument"; return JASPER_ERR; }
    uint8_t *const out[3] = {out0, out1, out2};
    double *const ds = device_seconds;
    RouteSeconds S = {0, 0, 0};
    int rc = -1;
    if (out_cap) {
        rc = gz_text_route(*h->g, t->t, want, RouteJob{n_seg, bounds, bins, first, check_from}, RouteOut{out, out_cap, out_bytes, raw_bytes, mismatches, counters}, got, S, g_err);
    } else {
        if (counters) std::fill(counters, counters + DF_COUNTERS, (uint64_t)0);
        g_err = "gz text: bad arguments";
    }
    if (ds) { ds[0] = S.route; ds[1] = S.pull; ds[2] = S.deflate; }
    return rc ? JASPER_ERR : JASPER_OK;
}

// ---- variant scan (variants.hip) ----
int jasper_variant_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_varscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), t, n_seqs, out, [&](jasper_varscan &r) { return variant_scan_host(t->t, n_seqs, seqs, lens, thre, r.r, g_err); });
}
int jasper_variant_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, jasper_varscan **out) {
    return scan_call(offsets, t, n_seqs, out, [&](jasper_varscan &r) { return variant_scan_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, r.r, g_err); });
}
int jasper_varscan_num_seqs(const jasper_varscan *r) { return r ? (int)(r->r.counts.size() / 3) : 0; }
int jasper_varscan_counts(const jasper_varscan *r, int seq, uint64_t out3[3]) { return counts_out<3>(r ? &r->r.counts : nullptr, seq, out3); }
int jasper_varscan_records(const jasper_varscan *r, const jasper_variant **recs, uint64_t *n) { return records_out(r ? &r->r.recs : nullptr, recs, n); }
int jasper_varscan_candidates(const jasper_varscan *r, uint64_t *n) { return word_out(r ? &r->r.candidates : nullptr, n); }
double jasper_varscan_seconds(const jasper_varscan *r) { return r ? r->r.seconds : 0.0; }
int jasper_varscan_retried(const jasper_varscan *r) { return r ? r->r.retried : 0; }
void jasper_varscan_free(jasper_varscan *r) { delete r; }

// ---- indel scan (indels.hip) ----
static_assert(offsetof(jasper_indel, len) == offsetof(Indel, len) && offsetof(jasper_indel, type) == offsetof(Indel, type) && offsetof(jasper_indel, base) == offsetof(Indel, base) &&
                  offsetof(jasper_indel, kind) == offsetof(Indel, kind),
              "jasper_indel is Indel");
static_assert(offsetof(jasper_mixed_ins, bases) == offsetof(MixedIns, bases) && offsetof(jasper_mixed_ins, len) == offsetof(MixedIns, len) &&
                  offsetof(jasper_mixed_ins, kind) == offsetof(MixedIns, kind),
              "jasper_mixed_ins is MixedIns");
static_assert(JASPER_INDEL_FRONT == INDEL_FRONT, "the header's cap is the kernel's");
static_assert(offsetof(jasper_het_cluster, alt_min) == offsetof(HetCluster, alt_min) && offsetof(jasper_het_cluster, ref_len) == offsetof(HetCluster, ref_len) &&
                  offsetof(jasper_het_cluster, bases) == offsetof(HetCluster, bases) && offsetof(jasper_het_cluster, len) == offsetof(HetCluster, len),
              "jasper_het_cluster is HetCluster");
// seqs / lens or d_text / offsets, whichever the entry point has.  cluster_len < 0: an entry point without clusters (the scan runs with 0);
// the cluster entry points pass max(cluster_len, 0), which has to be in 1..CLUSTER_MAX_LEN -- checked after the text arguments, as before.
static int indelscan_call(bool args_ok, jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, const void *d_text, const int64_t *offsets, uint32_t thre,
                          int max_len, bool mixed, int cluster_len, jasper_indelscan **out) {
    if (args_ok && cluster_len >= 0 && (cluster_len < 1 || cluster_len > CLUSTER_MAX_LEN)) { g_err = "indel scan: cluster_len must be in 1..64"; return JASPER_ERR; }
    const int cl = std::max(cluster_len, 0);
    return scan_call(args_ok, t, n_seqs, out, [&](jasper_indelscan &r) {
        const int rc = offsets ? indel_scan_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, max_len, mixed, cl, r.r, g_err)
                               : indel_scan_host(t->t, n_seqs, seqs, lens, thre, max_len, mixed, cl, r.r, g_err);
        r.var.r = std::move(r.r.var);
        return rc;
    });
}
int jasper_indel_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_indelscan **out) {
    return indelscan_call(host_args(n_seqs, seqs, lens), t, n_seqs, seqs, lens, nullptr, nullptr, thre, max_len, false, -1, out);
}
int jasper_indel_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_indelscan **out) {
    return indelscan_call(offsets, t, n_seqs, nullptr, nullptr, d_text, offsets, thre, max_len, false, -1, out);
}
int jasper_indel_scan_mixed(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_indelscan **out) {
    return indelscan_call(host_args(n_seqs, seqs, lens), t, n_seqs, seqs, lens, nullptr, nullptr, thre, max_len, true, -1, out);
}
int jasper_indel_scan_mixed_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_indelscan **out) {
    return indelscan_call(offsets, t, n_seqs, nullptr, nullptr, d_text, offsets, thre, max_len, true, -1, out);
}
int jasper_indel_scan_clusters(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int mixed, int cluster_len,
                               jasper_indelscan **out) {
    return indelscan_call(host_args(n_seqs, seqs, lens), t, n_seqs, seqs, lens, nullptr, nullptr, thre, max_len, mixed != 0, std::max(cluster_len, 0), out);
}
int jasper_indel_scan_clusters_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, int mixed, int cluster_len,
                                      jasper_indelscan **out) {
    return indelscan_call(offsets, t, n_seqs, nullptr, nullptr, d_text, offsets, thre, max_len, mixed != 0, std::max(cluster_len, 0), out);
}
int jasper_indelscan_num_seqs(const jasper_indelscan *r) { return r ? (int)(r->r.counts.size() / 4) : 0; }
int jasper_indelscan_counts(const jasper_indelscan *r, int seq, uint64_t out4[4]) { return counts_out<4>(r ? &r->r.counts : nullptr, seq, out4); }
int jasper_indelscan_records(const jasper_indelscan *r, const jasper_indel **recs, uint64_t *n) { return records_out(r ? &r->r.recs : nullptr, recs, n); }
const jasper_varscan *jasper_indelscan_variants(const jasper_indelscan *r) { return r ? &r->var : nullptr; }
double jasper_indelscan_seconds(const jasper_indelscan *r) { return r ? r->r.seconds : 0.0; }
double jasper_indelscan_check_seconds(const jasper_indelscan *r) { return r ? r->r.check_seconds : 0.0; }
int jasper_indelscan_lookups(const jasper_indelscan *r, uint64_t *n) { return word_out(r ? &r->r.lookups : nullptr, n); }
int jasper_indelscan_retried(const jasper_indelscan *r) { return r ? r->r.retried : 0; }
int jasper_indelscan_mixed_counts(const jasper_indelscan *r, int seq, uint64_t out3[3]) {
    return counts_out<3>(r ? &r->r.mixed_counts : nullptr, r ? r->r.counts.size() / 4 : 0, seq, out3);
}
int jasper_indelscan_mixed_records(const jasper_indelscan *r, const jasper_mixed_ins **recs, uint64_t *n) { return records_out(r ? &r->r.mixed_recs : nullptr, recs, n); }
double jasper_indelscan_mixed_seconds(const jasper_indelscan *r) { return r ? r->r.mixed_seconds : 0.0; }
int jasper_indelscan_mixed_lookups(const jasper_indelscan *r, uint64_t *n) { return word_out(r ? &r->r.mixed_lookups : nullptr, n); }
int jasper_indelscan_mixed_retried(const jasper_indelscan *r) { return r ? r->r.mixed_retried : 0; }
int jasper_indel_front(void) { return INDEL_FRONT; }
int jasper_indelscan_cluster_counts(const jasper_indelscan *r, int seq, uint64_t out4[4]) {
    return counts_out<4>(r ? &r->r.cluster_counts : nullptr, r ? r->r.counts.size() / 4 : 0, seq, out4);
}
int jasper_indelscan_cluster_records(const jasper_indelscan *r, const jasper_het_cluster **recs, uint64_t *n) {
    return records_out(r ? &r->r.cluster_recs : nullptr, recs, n);
}
double jasper_indelscan_cluster_seconds(const jasper_indelscan *r) { return r ? r->r.cluster_seconds : 0.0; }
int jasper_indelscan_cluster_lookups(const jasper_indelscan *r, uint64_t *n) { return word_out(r ? &r->r.cluster_lookups : nullptr, n); }
int jasper_indelscan_cluster_retried(const jasper_indelscan *r) { return r ? r->r.cluster_retried : 0; }
void jasper_indelscan_free(jasper_indelscan *r) { delete r; }

// ---- compound scan (compound.hip) ----
static_assert(offsetof(jasper_compound, ref_len) == offsetof(Compound, ref_len) && offsetof(jasper_compound, bases) == offsetof(Compound, bases) &&
                  offsetof(jasper_compound, len) == offsetof(Compound, len),
              "jasper_compound is Compound");
static_assert(sizeof(jasper_compound) == 48, "jasper_compound is 48 bytes");
static_assert(JASPER_COMPOUND_FRONT == COMPOUND_FRONT && COMPOUND_FRONT == INDEL_FRONT, "the header's cap is the kernel's, and the mixed search's");
int jasper_compound_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_compscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), t, n_seqs, out,
                     [&](jasper_compscan &r) { return compound_scan_host(t->t, n_seqs, seqs, lens, thre, max_len, r.rep.r, r.r, g_err); });
}
int jasper_compound_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_compscan **out) {
    return scan_call(offsets, t, n_seqs, out,
                     [&](jasper_compscan &r) { return compound_scan_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, max_len, r.rep.r, r.r, g_err); });
}
int jasper_compscan_num_seqs(const jasper_compscan *r) { return r ? (int)(r->r.counts.size() / 5) : 0; }
int jasper_compscan_counts(const jasper_compscan *r, int seq, uint64_t out5[5]) { return counts_out<5>(r ? &r->r.counts : nullptr, seq, out5); }
int jasper_compscan_records(const jasper_compscan *r, const jasper_compound **recs, uint64_t *n) { return records_out(r ? &r->r.recs : nullptr, recs, n); }
const jasper_report *jasper_compscan_report(const jasper_compscan *r) { return r ? &r->rep : nullptr; }
int jasper_compscan_lookups(const jasper_compscan *r, uint64_t *n) { return word_out(r ? &r->r.lookups : nullptr, n); }
int jasper_compscan_seconds(const jasper_compscan *r, double *search, double *total) {
    if (!r) { g_err = "bad argument"; return JASPER_ERR; }
    if (search) *search = r->r.search_seconds;
    if (total) *total = r->r.seconds;
    return JASPER_OK;
}
int jasper_compscan_retried(const jasper_compscan *r) { return r ? r->r.retried : 0; }
int jasper_compound_front(void) { return COMPOUND_FRONT; }
void jasper_compscan_free(jasper_compscan *r) { delete r; }

// ---- repair (repair.hip) ----
static_assert(offsetof(jasper_edit, ref_len) == offsetof(Edit, ref_len) && offsetof(jasper_edit, bases) == offsetof(Edit, bases) && offsetof(jasper_edit, len) == offsetof(Edit, len) &&
                  offsetof(jasper_edit, source) == offsetof(Edit, source) && offsetof(jasper_edit, round) == offsetof(Edit, round),
              "jasper_edit is Edit");
static_assert(sizeof(jasper_edit) == 48 && sizeof(jasper_repair_round) == sizeof(RepairRound), "public and host record layouts must match");
int jasper_repair(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int indel_max_len, int compound_max_len, int rounds,
                  jasper_repaired **out) {
    return repair_call(host_args(n_seqs, seqs, lens), t, n_seqs, out,
                       [&](RepairOut &r) { return repair_host(t->t, n_seqs, seqs, lens, thre, indel_max_len, compound_max_len, rounds, r, g_err); });
}
int jasper_repair_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int indel_max_len, int compound_max_len, int rounds,
                         jasper_repaired **out) {
    return repair_call(offsets, t, n_seqs, out,
                       [&](RepairOut &r) { return repair_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, indel_max_len, compound_max_len, rounds, r, g_err); });
}
int jasper_apply_edits(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, const jasper_edit *edits, uint64_t n_edits, jasper_repaired **out) {
    return repair_call(host_args(n_seqs, seqs, lens), t, n_seqs, out,
                       [&](RepairOut &r) { return apply_edits_host(t->t, n_seqs, seqs, lens, reinterpret_cast<const Edit *>(edits), n_edits, r, g_err); });
}
int jasper_apply_edits_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, const jasper_edit *edits, uint64_t n_edits,
                              jasper_repaired **out) {
    return repair_call(offsets, t, n_seqs, out, [&](RepairOut &r) {
        return apply_edits_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, reinterpret_cast<const Edit *>(edits), n_edits, r, g_err);
    });
}
int jasper_repair_tile_bytes(void) { return REPAIR_TILE; }
int jasper_repaired_num_seqs(const jasper_repaired *r) { return r && !r->r.offsets.empty() ? (int)(r->r.offsets.size() - 1) : 0; }
int jasper_repaired_seq(const jasper_repaired *r, int seq, const char **text, int64_t *len) {
    if (!r || !text || !len || seq < 0 || (size_t)seq + 1 >= r->r.offsets.size()) { g_err = "bad argument"; return JASPER_ERR; }
    *text = r->r.text.data() + r->r.offsets[seq];
    *len = r->r.offsets[seq + 1] - r->r.offsets[seq];
    return JASPER_OK;
}
int jasper_repaired_edits(const jasper_repaired *r, const jasper_edit **edits, uint64_t *n) { return records_out(r ? &r->r.edits : nullptr, edits, n); }
int jasper_repaired_rounds(const jasper_repaired *r, const jasper_repair_round **rounds, uint64_t *n) { return records_out(r ? &r->r.rounds : nullptr, rounds, n); }
const jasper_report *jasper_repaired_before(const jasper_repaired *r) { return r ? &r->before : nullptr; }
const jasper_report *jasper_repaired_after(const jasper_repaired *r) { return r ? &r->after : nullptr; }
int jasper_repaired_seconds(const jasper_repaired *r, double *apply, double *total) {
    if (!r) { g_err = "bad argument"; return JASPER_ERR; }
    if (apply) *apply = r->r.apply_seconds;
    if (total) *total = r->r.seconds;
    return JASPER_OK;
}
void jasper_repaired_free(jasper_repaired *r) { delete r; }

// ---- gap scan (gaps.hip) ----
static_assert(offsetof(jasper_gap_site, q) == offsetof(GapSite, q) && offsetof(jasper_gap_site, seq) == offsetof(GapSite, seq) &&
                  offsetof(jasper_gap_site, ref_min) == offsetof(GapSite, ref_min) && offsetof(jasper_gap_site, n_records) == offsetof(GapSite, n_records) &&
                  offsetof(jasper_gap_site, levels) == offsetof(GapSite, levels) && offsetof(jasper_gap_site, trim_left) == offsetof(GapSite, trim_left) &&
                  offsetof(jasper_gap_site, trim_right) == offsetof(GapSite, trim_right) && offsetof(jasper_gap_site, kind) == offsetof(GapSite, kind) &&
                  offsetof(jasper_gap_site, status) == offsetof(GapSite, status),
              "jasper_gap_site is GapSite");
static_assert(offsetof(jasper_gap_fill, bases_off) == offsetof(GapFill, bases_off) && offsetof(jasper_gap_fill, seq) == offsetof(GapFill, seq) &&
                  offsetof(jasper_gap_fill, ref_len) == offsetof(GapFill, ref_len) && offsetof(jasper_gap_fill, len) == offsetof(GapFill, len) &&
                  offsetof(jasper_gap_fill, alt_min) == offsetof(GapFill, alt_min),
              "jasper_gap_fill is GapFill");
static_assert(sizeof(jasper_gap_site) == 48 && sizeof(jasper_gap_fill) == 32, "jasper_gap_site is 48 bytes, jasper_gap_fill 32");
static_assert(JASPER_GAP_FRONT == GAP_FRONT && JASPER_GAP_MAX_RECORDS == GAP_MAX_RECORDS && JASPER_GAP_MAX_LEN == GAP_MAX_LEN && JASPER_GAP_RUN_MIN == GAP_RUN_MIN &&
                  JASPER_GAP_SKIPPED == GAP_SKIPPED && JASPER_GAP_KIND_RUN == GAP_KIND_RUN,
              "the header's constants are the kernel's");
int jasper_gap_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int64_t max_trim, int long_runs,
                    jasper_gapscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), t, n_seqs, out,
                     [&](jasper_gapscan &r) { return gap_scan_host(t->t, n_seqs, seqs, lens, thre, max_len, max_trim, long_runs != 0, r.rep.r, r.r, g_err); });
}
int jasper_gap_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, int64_t max_trim, int long_runs,
                           jasper_gapscan **out) {
    return scan_call(offsets, t, n_seqs, out, [&](jasper_gapscan &r) {
        return gap_scan_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, max_len, max_trim, long_runs != 0, r.rep.r, r.r, g_err);
    });
}
int jasper_gap_search(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, const jasper_gap_site *sites, uint64_t n_sites,
                      jasper_gapscan **out) {
    return scan_call(host_args(n_seqs, seqs, lens), t, n_seqs, out, [&](jasper_gapscan &r) {
        return gap_search_host(t->t, n_seqs, seqs, lens, thre, max_len, reinterpret_cast<const GapSite *>(sites), n_sites, r.r, g_err);
    });
}
int jasper_gap_search_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, const jasper_gap_site *sites,
                             uint64_t n_sites, jasper_gapscan **out) {
    return scan_call(offsets, t, n_seqs, out, [&](jasper_gapscan &r) {
        return gap_search_device(t->t, n_seqs, (const uint8_t *)d_text, offsets, thre, max_len, reinterpret_cast<const GapSite *>(sites), n_sites, r.r, g_err);
    });
}
int jasper_gapscan_num_seqs(const jasper_gapscan *r) { return r ? (int)(r->r.counts.size() / GAP_COUNTS) : 0; }
int jasper_gapscan_counts(const jasper_gapscan *r, int seq, uint64_t out9[9]) { return counts_out<GAP_COUNTS>(r ? &r->r.counts : nullptr, seq, out9); }
int jasper_gapscan_sites(const jasper_gapscan *r, const jasper_gap_site **sites, uint64_t *n) { return records_out(r ? &r->r.sites : nullptr, sites, n); }
int jasper_gapscan_records(const jasper_gapscan *r, const jasper_gap_fill **recs, uint64_t *n) { return records_out(r ? &r->r.fills : nullptr, recs, n); }
int jasper_gapscan_bases(const jasper_gapscan *r, const char **bases, uint64_t *n) {
    if (!r || !bases || !n) { g_err = "bad argument"; return JASPER_ERR; }
    *bases = r->r.pool.data();
    *n = r->r.pool.size();
    return JASPER_OK;
}
const jasper_report *jasper_gapscan_report(const jasper_gapscan *r) { return r ? &r->rep : nullptr; }
int jasper_gapscan_seconds(const jasper_gapscan *r, double *search, double *runs, double *total) {
    if (!r) { g_err = "bad argument"; return JASPER_ERR; }
    if (search) *search = r->r.search_seconds;
    if (runs) *runs = r->r.runs_seconds;
    if (total) *total = r->r.seconds;
    return JASPER_OK;
}
int jasper_gapscan_lookups(const jasper_gapscan *r, uint64_t *n) { return word_out(r ? &r->r.lookups : nullptr, n); }
int jasper_gapscan_retried(const jasper_gapscan *r) { return r ? r->r.retried : 0; }
int jasper_gap_front(void) { return GAP_FRONT; }
int jasper_gap_max_records(void) { return GAP_MAX_RECORDS; }
int jasper_gap_max_len(void) { return GAP_MAX_LEN; }
void jasper_gapscan_free(jasper_gapscan *r) { delete r; }

}  // extern "C"
