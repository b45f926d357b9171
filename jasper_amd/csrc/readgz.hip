// readgz.hip -- the host stage of a gzip text session (readgz.hpp): no kernel of its own.  It moves text between the inflater's buffer,
// the session's tail buffer and the slot the read-text or routing kernels read, always between distinct buffers, on the table's stream.
#include "readgz.hpp"
#include "deflate_plan.hpp"
#include "scan_tile.hpp"

namespace jk {

namespace {
const char *const GZ_WHAT = "gz text";

// up to `want` inflated bytes to d_dst, timed by HIP events (the pair is read once the stream has been waited for) -> got, or -1
long pull(GzText &G, uint8_t *d_dst, int64_t want, Events &ev, std::string &err) {
    hipStream_t st = G.M->stream;
    if (hipEventRecord(ev.e[0], st) != hipSuccess) { err = std::string(GZ_WHAT) + ": hipEventRecord"; return -1; }
    const long got = G.dg->read_device(d_dst, (size_t)want);
    if (got < 0) { err = G.dg->err; return -1; }
    if (hipEventRecord(ev.e[1], st) != hipSuccess) { err = std::string(GZ_WHAT) + ": hipEventRecord"; return -1; }
    return got;
}
}  // namespace

GzText::~GzText() {
    if (M) {
        (void)hipSetDevice(M->device);
        (void)jk_stream_wait(M->stream);
    }
    dg.reset();
    if (d_tail) (void)hipFree(d_tail);
}

GzText *gz_text_open(Table &M, const char *path, std::string &err) {
    const std::string w(GZ_WHAT);
    if (!path) { err = w + ": bad arguments"; return nullptr; }
    if (hipSetDevice(M.device) != hipSuccess) { err = w + ": hipSetDevice"; return nullptr; }
    std::unique_ptr<GzText> G(new GzText);
    G->M = &M;
    G->dg.reset(new DeviceGunzip(path, M.device, M.stream, GzdConfig::from_env(), G->stats));
    std::string e;
    Table *t = &M;
    if (!G->dg->open([t, &e](int slot, size_t bytes) { return t->workspace(Table::WS_GZ + slot, bytes, e); })) {
        err = w + ": " + path + " is not for the device inflater (not a regular file with a gzip header, or no device memory)" + (e.empty() ? "" : ": " + e);
        return nullptr;
    }
    return G.release();
}

int gz_text_bins(GzText &G, Table &M, Table &P, int64_t want, int *format, uint32_t thre_mat, uint32_t thre_pat, int64_t *n, int *eof, int64_t *used, int64_t *n_records,
                 int *status, int64_t *bad_record, double *seconds, std::string &err) {
    const std::string w(GZ_WHAT);
    if (!format || !n || !eof || want < 0 || *format < 0 || *format > 2) { err = w + ": bad arguments"; return -1; }
    if (&M != G.M) { err = w + ": the maternal table is not the one the session was opened on"; return -1; }
    if (G.mode == 2) { err = w + ": the session has routed; a pass over the file is bins calls or route calls, not both"; return -1; }
    *n = 0;
    *eof = 0;
    if (seconds) seconds[2] = 0;
    if (read_text_check(M, P, 0, RT_FASTQ, thre_mat, thre_pat, used, n_records, status, bad_record, seconds, err)) return -1;
    if (G.tail + want > RT_MAX_TEXT) { err = w + ": the carried tail and want are more than 2^31-1 text bytes in one call"; return -1; }      // (before anything is inflated)
    HIPCHK(hipSetDevice(M.device));
    hipStream_t st = M.stream;
    G.n = -1;
    G.mode = 1;
    uint8_t *d_text = (uint8_t *)M.workspace(Table::WS_READTEXT, (size_t)(G.tail + want) + RT_PAD, err);
    if (!d_text) return -1;
    if (G.tail) HIPCHK(hipMemcpyAsync(d_text, G.d_tail, (size_t)G.tail, hipMemcpyDeviceToDevice, st));
    Events ev;
    if (ev.create(err)) return -1;
    const long got = pull(G, d_text + G.tail, want, ev, err);
    if (got < 0) return -1;
    const int64_t total = G.tail + got;
    const int at_end = got < want || G.dg->at_end();
    int fmt = *format;
    uint8_t first = 0;
    if (fmt == 0 && total) {                            // (the first call alone)
        HIPCHK(hipMemcpyAsync(&first, d_text, 1, hipMemcpyDeviceToHost, st));
        HIPCHK(jk_stream_wait(st));
        fmt = first == '@' ? 1 : first == '>' ? 2 : 0;
    }
    G.n = total;
    *n = total;
    *eof = at_end;
    int rc = 0;
    if (fmt == 0) {
        if (total) *status = RT_NO_FORMAT;              // (nothing is parsed: the whole text stays the tail)
        M.text_records = 0; M.text_seq_bytes = 0; M.text_used = 0;
    } else {
        *format = fmt;
        double s2[2] = {0, 0};
        rc = read_text_core(M, P, total, at_end, fmt - 1, -1, thre_mat, thre_pat, used, n_records, status, bad_record, s2, err);
        if (seconds) { seconds[0] = s2[0]; seconds[1] = s2[1]; }
    }
    if (fmt == 0 || total == 0) HIPCHK(jk_stream_wait(st));      // (otherwise the core has waited behind the inflater's second event)
    if (!rc && seconds && ev.add_seconds(seconds[2], err)) return -1;
    if (rc) return rc;
    // the tail for the next call
    const int64_t keep_from = *status == RT_CLEAN ? *used : 0, keep = total - keep_from;
    if (keep > 0) {
        if ((size_t)keep > G.tail_cap) {
            HIPCHK(jk_stream_wait(st));                 // (the copy out of the old tail buffer has ended)
            if (G.d_tail) (void)hipFree(G.d_tail);
            G.d_tail = nullptr;
            G.tail_cap = 0;
            const size_t cap = (size_t)keep + (size_t)keep / 2 + 4096;
            HIPCHK(hipMalloc((void **)&G.d_tail, cap));
            G.tail_cap = cap;
        }
        HIPCHK(hipMemcpyAsync(G.d_tail, d_text + keep_from, (size_t)keep, hipMemcpyDeviceToDevice, st));
    }
    G.tail = keep;
    return 0;
}

int gz_text_copy(GzText &G, int64_t from, int64_t len, uint8_t *dst, std::string &err) {
    const std::string w(GZ_WHAT);
    if (G.n < 0) { err = w + ": no call has left a text to copy from"; return -1; }
    if (from < 0 || len < 0 || from > G.n || len > G.n - from || (len && !dst)) { err = w + ": the bytes asked for are not all in the current text"; return -1; }
    if (len == 0) return 0;
    Table &M = *G.M;
    HIPCHK(hipSetDevice(M.device));
    HIPCHK(hipMemcpyAsync(dst, (const uint8_t *)M.ws[Table::WS_READTEXT].p + from, (size_t)len, hipMemcpyDeviceToHost, M.stream));
    HIPCHK(jk_stream_wait(M.stream));
    return 0;
}

// the arguments, the session's mode, the outputs' initial state, the pull of the next `want` inflated bytes into the routing path's text
// slot, and route_text on them where they are
int gz_text_route(GzText &G, Table &T, int64_t want, const RouteJob &J, const RouteOut &O, int64_t *got, RouteSeconds &S, std::string &err) {
    const std::string w(GZ_WHAT);
    S = RouteSeconds{0, 0, 0};
    if (O.out_cap) {
        if (O.counters)
            for (int i = 0; i < DF_COUNTERS; ++i) O.counters[i] = 0;
        if (!O.raw_bytes) { err = w + ": bad arguments"; return -1; }
        O.raw_bytes[0] = O.raw_bytes[1] = O.raw_bytes[2] = 0;
    }
    if (!got || !O.out_bytes || !O.mismatches || !J.bounds || J.n_seg < 0 || want < 0) { err = w + ": bad arguments"; return -1; }
    if (&T != G.M) { err = w + ": the table is not the one the session was opened on"; return -1; }
    if (G.mode == 1) { err = w + ": the session has served bins calls; a pass over the file is bins calls or route calls, not both"; return -1; }
    G.mode = 2;
    *got = 0;
    *O.mismatches = 0;
    O.out_bytes[0] = O.out_bytes[1] = O.out_bytes[2] = 0;
    HIPCHK(hipSetDevice(T.device));
    uint8_t *d_text = route_text_room(T, want, err);
    if (!d_text) return -1;
    Events ev;
    if (ev.create(err)) return -1;
    const long g = pull(G, d_text, want, ev, err);
    if (g < 0) return -1;
    HIPCHK(jk_stream_wait(T.stream));
    if (ev.add_seconds(S.pull, err)) return -1;
    *got = g;
    if (*got != J.bounds[J.n_seg]) return 0;            // (the file is not what the bounds were made for: nothing is routed)
    return route_text(T, d_text, true, *got, J, O, S, err);
}

}  // namespace jk
