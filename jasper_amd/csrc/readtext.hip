// readtext.hip -- a chunk of raw FASTQ / FASTA text in HBM -> its records' sequences packed back to back, the n + 1 offsets
// read_bins_kernel takes and the small per-record arrays the host names and routes the records by (semantics: include/jasper_hip.h,
// jasper_read_text_bins; the host parser it restates: jasper_amd/triobin.py).
//
// An extension the reference has no counterpart for, and a path of its own beside the read feed (ingest_gpu.hip), which marks a record's
// end inside the base stream and hands out no offsets.  The cut into kernels follows that file's: line feeds per block, a scan, one
// position per line; then everything is per LINE, so that the two formats differ in one kernel only.
//
//   rt_count_lf_kernel   line feeds per block of RT_BLOCK text bytes (16 per thread, one 16-byte load)
//   rt_scan_tops_kernel  exclusive scan of block totals in place, the total behind them: ONE workgroup, RT_SCAN_PASS totals a pass with
//                        the running sum carried from pass to pass
//   rt_nlpos_kernel      nlpos[line] = where line `line` ends (its line feed; at the end of the file the text's end for a last line
//                        without one).  Line `line` begins at nlpos[line - 1] + 1
//   rt_lines_kernel      one thread per line: val[line] = the stripped length (a CR right before the line's end is not part of it) of a
//                        SEQUENCE line, 2^32 for a FASTA header, else 0.  FASTQ: the record's shape is checked here -- '@', '+', quality as
//                        long as sequence -- and the first record that fails is found by an atomicMin
//   rt_scan_reduce_kernel, rt_scan_tops_kernel, rt_scan_apply_kernel
//                        pre = exclusive scan of val with the total behind it: its low word is where a line's bytes go in the packed
//                        sequences (line_out), its high word the number of FASTA headers before the line (a header's record)
//   rt_records_kernel    one thread per line: a record's first line writes rec_start, head_end and offsets of its record; the tail
//                        (rec_start[n] = used, offsets[n], the span read_bins_kernel reads behind the offsets) by the line that knows it
//   rt_pack_kernel       by TEXT bytes, 16 per thread: a block recomputes its line-feed rank from the block base, a byte of a sequence
//                        line goes to line_out[line] + (pos - line start).  A 100 kb line of a long read is spread over many workgroups
//                        this way.  16 bytes inside one line leave in one 16-byte store
//   rt_lens_kernel       lens[i] = offsets[i + 1] - offsets[i]
// The host stage waits three times: for the line-feed total (it sizes the line arrays), for the scan's total and the first bad record
// (they size the record arrays, and nothing is binned of a malformed chunk), and for `used` and the packed bytes (the binning's tiles).
#include "readtext.hpp"
#include "readbins.hpp"
#include "hapmers.hpp"
#include "scan_tile.hpp"

namespace jk {

namespace {

constexpr uint64_t RT_HEADER = 1ull << 32;      // val of a FASTA header line
enum { RTC_BAD = 0, RTC_USED = 1, RTC_BYTES = 2, RTC_WORDS = 4 };      // control words (uint64): first bad record, used, packed bytes

__device__ __forceinline__ uint32_t byte_of(const Raw16 &r, int j) { return (r.w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }
__device__ __forceinline__ uint32_t count_lf(const Raw16 &r, uint64_t pos, uint64_t n) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) c += (pos + j < n && byte_of(r, j) == '\n');
    return c;
}

// exclusive prefix of v over the workgroup (THREADS a multiple of 64) and the workgroup's total; s_w holds THREADS / 64 words
template <int THREADS>
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t *s_w, uint64_t &total) {
    const int t = threadIdx.x;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)inc, o);
        if ((t & 63) >= o) inc += u;
    }
    if ((t & 63) == 63) s_w[t >> 6] = inc;
    __syncthreads();
    uint64_t wbase = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const uint64_t x = s_w[w];
        if (w < (t >> 6)) wbase += x;
        total += x;
    }
    __syncthreads();
    return wbase + inc - v;
}

__global__ __launch_bounds__(RT_THREADS) void rt_count_lf_kernel(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ blk) {
    __shared__ uint64_t s_w[RT_THREADS / 64];
    const uint64_t pos = (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16;
    uint32_t c = 0;
    if (pos < n) c = count_lf(load16(text, (int64_t)pos, (int64_t)n), pos, n);
    uint64_t total;
    (void)block_exclusive<RT_THREADS>(c, s_w, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// tot[0 .. nb) -> their exclusive sums, tot[nb] = the total
__global__ __launch_bounds__(RT_SCAN_PASS) void rt_scan_tops_kernel(uint64_t *__restrict__ tot, uint64_t nb) {
    __shared__ uint64_t s_w[RT_SCAN_PASS / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += RT_SCAN_PASS) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? tot[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive<RT_SCAN_PASS>(v, s_w, total);
        if (i < nb) tot[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tot[nb] = carry;
}

// virt: the line that ends at the text's end without a line feed, or ~0
__global__ __launch_bounds__(RT_THREADS) void rt_nlpos_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ blk, uint32_t virt,
                                                              uint32_t *__restrict__ nlpos) {
    __shared__ uint64_t s_w[RT_THREADS / 64];
    const uint64_t pos = (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16;
    Raw16 r;
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0;
    uint32_t c = 0;
    if (pos < n) {
        r = load16(text, (int64_t)pos, (int64_t)n);
        c = count_lf(r, pos, n);
    }
    uint64_t total;
    uint32_t line = (uint32_t)(blk[blockIdx.x] + block_exclusive<RT_THREADS>(c, s_w, total));
    if (c)
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (pos + j < n && byte_of(r, j) == '\n') nlpos[line++] = (uint32_t)(pos + j);
    if (blockIdx.x == 0 && threadIdx.x == 0 && virt != 0xFFFFFFFFu) nlpos[virt] = (uint32_t)n;
}

struct Line { uint32_t s, e; };     // [s, e): the line without its line end (CR LF, LF, or a CR before the text's end)
__device__ __forceinline__ Line line_of(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nlpos, uint32_t line) {
    Line l;
    l.s = line ? nlpos[line - 1] + 1 : 0u;
    l.e = nlpos[line];
    if (l.e > l.s && text[l.e - 1] == '\r') --l.e;
    return l;
}

// nl lines (FASTQ: 4 per record, whole records only)
__global__ __launch_bounds__(RT_THREADS) void rt_lines_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nlpos, uint32_t nl, int format,
                                                              uint64_t *__restrict__ val, unsigned long long *__restrict__ ctl) {
    const uint32_t line = blockIdx.x * RT_THREADS + threadIdx.x;
    if (line >= nl) return;
    const Line l = line_of(text, nlpos, line);
    const uint32_t first = text[l.s];                   // (of an empty line: its line end, which is none of @ + >)
    uint64_t v = 0;
    if (format == RT_FASTA) {
        v = first == '>' ? RT_HEADER : (uint64_t)(l.e - l.s);
    } else {
        const uint32_t j = line & 3u;
        bool bad = false;
        if (j == 0) bad = first != '@';
        else if (j == 1) v = l.e - l.s;
        else if (j == 2) bad = first != '+';
        else {
            const Line q = line_of(text, nlpos, line - 2);
            bad = l.e - l.s != q.e - q.s;
        }
        if (bad) atomicMin(&ctl[RTC_BAD], (unsigned long long)(line >> 2));
    }
    val[line] = v;
}

// the scan of n words in blocks of RT_BLOCK: a thread's 16 words are consecutive
__device__ __forceinline__ uint64_t load_words16(const uint64_t *__restrict__ in, uint64_t n, uint64_t at, uint64_t w[16]) {
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        w[j] = at + j < n ? in[at + j] : 0;
        sum += w[j];
    }
    return sum;
}
__global__ __launch_bounds__(RT_THREADS) void rt_scan_reduce_kernel(const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ blk) {
    __shared__ uint64_t s_w[RT_THREADS / 64];
    uint64_t w[16], total;
    (void)block_exclusive<RT_THREADS>(load_words16(in, n, (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16, w), s_w, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}
// out[i] = the sum of in[0 .. i) for i <= n
__global__ __launch_bounds__(RT_THREADS) void rt_scan_apply_kernel(const uint64_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ blk, uint64_t *__restrict__ out) {
    __shared__ uint64_t s_w[RT_THREADS / 64];
    const uint64_t at = (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16;
    uint64_t w[16], total;
    const uint64_t mine = load_words16(in, n, at, w);
    uint64_t run = blk[blockIdx.x] + block_exclusive<RT_THREADS>(mine, s_w, total);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (at + j <= n) out[at + j] = run;             // (the entry behind the last word is the total)
        run += w[j];
    }
}

// rec: rec_start[n_rec + 1], head_end[n_rec]; offs: n_rec + 1 offsets and the span {0, offs[n_rec]}.  FASTA: the header of rank n_rec,
// where there is one (the chunk does not end the file), is where the used text ends.
__global__ __launch_bounds__(RT_THREADS) void rt_records_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ nlpos, uint32_t nl, int format,
                                                                int tail_at_end, const uint64_t *__restrict__ val, const uint64_t *__restrict__ pre, uint64_t n_rec,
                                                                int64_t *__restrict__ rec, int64_t *__restrict__ offs, unsigned long long *__restrict__ ctl) {
    const uint32_t line = blockIdx.x * RT_THREADS + threadIdx.x;
    if (line >= nl) return;
    int64_t *rec_start = rec, *head_end = rec + n_rec + 1;
    if (line == 0 && tail_at_end) {
        const uint64_t used = min((uint64_t)nlpos[nl - 1] + 1, n), bytes = pre[nl] & 0xFFFFFFFFull;
        rec_start[n_rec] = (int64_t)used;
        offs[n_rec] = (int64_t)bytes;
        offs[n_rec + 1] = 0;
        offs[n_rec + 2] = (int64_t)bytes;
        ctl[RTC_USED] = used;
        ctl[RTC_BYTES] = bytes;
    }
    uint64_t r;
    if (format == RT_FASTA) {
        if (val[line] != RT_HEADER) return;
        r = pre[line] >> 32;
    } else {
        if (line & 3u) return;
        r = line >> 2;
    }
    if (r > n_rec) return;
    const Line l = line_of(text, nlpos, line);
    const uint64_t bytes = pre[line] & 0xFFFFFFFFull;
    rec_start[r] = l.s;
    offs[r] = (int64_t)bytes;
    if (r < n_rec) {
        head_end[r] = l.e;
    } else if (!tail_at_end) {
        offs[n_rec + 1] = 0;
        offs[n_rec + 2] = (int64_t)bytes;
        ctl[RTC_USED] = l.s;
        ctl[RTC_BYTES] = bytes;
    }
}

__global__ __launch_bounds__(RT_THREADS) void rt_pack_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ blk, const uint32_t *__restrict__ nlpos,
                                                             int format, const uint64_t *__restrict__ val, const uint64_t *__restrict__ pre,
                                                             const unsigned long long *__restrict__ ctl, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_w[RT_THREADS / 64];
    const uint64_t used = ctl[RTC_USED];                // (bytes before it lie in lines the line kernels have looked at)
    const uint64_t pos = (uint64_t)blockIdx.x * RT_BLOCK + (uint64_t)threadIdx.x * 16;
    Raw16 r;
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0;
    uint32_t c = 0;
    if (pos < n) {
        r = load16(text, (int64_t)pos, (int64_t)n);
        c = count_lf(r, pos, n);
    }
    uint64_t total;
    uint32_t line = (uint32_t)(blk[blockIdx.x] + block_exclusive<RT_THREADS>(c, s_w, total));
    if (pos >= used) return;
    // the line my first byte lies in: its sequence bytes are [s, e) and go to out + dst
    uint32_t s = 0, e = 0;
    uint64_t dst = 0;
    auto open_line = [&]() {
        const uint64_t v = val[line];
        const bool seq = format == RT_FASTA ? v < RT_HEADER : (line & 3u) == 1u;
        s = line ? nlpos[line - 1] + 1 : 0u;
        e = seq ? s + (uint32_t)v : s;
        dst = pre[line] & 0xFFFFFFFFull;
    };
    open_line();
    if (pos >= s && pos + 16 <= e) {                    // (no line feed among them: e is before the line's)
        struct __attribute__((packed, aligned(1))) V16 { uint32_t w[4]; };
        V16 v;
        v.w[0] = r.w[0]; v.w[1] = r.w[1]; v.w[2] = r.w[2]; v.w[3] = r.w[3];
        *reinterpret_cast<V16 *>(out + dst + (pos - s)) = v;
        return;
    }
    for (int j = 0; j < 16; ++j) {
        const uint64_t p = pos + j;
        if (p >= used) break;
        const uint32_t b = byte_of(r, j);
        if (p >= s && p < e) out[dst + (p - s)] = (uint8_t)b;
        if (b == '\n') {
            ++line;
            if (p + 1 < used) open_line();
            else break;
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void rt_lens_kernel(const int64_t *__restrict__ offs, uint64_t n_rec, int64_t *__restrict__ lens) {
    const uint64_t i = (uint64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (i < n_rec) lens[i] = offs[i + 1] - offs[i];
}

const char *const RT_WHAT = "read text bins";

}  // namespace

// what both entries refuse, and the state they start from
int read_text_check(Table &M, Table &P, int64_t n, int format, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status, int64_t *bad_record,
                    double *seconds, std::string &err) {
    const std::string w(RT_WHAT);
    if (!used || !n_records || !status || !bad_record) { err = w + ": bad arguments"; return -1; }
    *used = *n_records = 0;
    *status = RT_CLEAN;
    *bad_record = -1;
    if (seconds) seconds[0] = seconds[1] = 0;
    M.text_records = -1;
    if (check_trio(RT_WHAT, M, P, nullptr, nullptr, thre_mat, thre_pat, 1, err)) return -1;
    if (n < 0 || (format != RT_FASTQ && format != RT_FASTA)) { err = w + ": bad arguments"; return -1; }
    if (n > RT_MAX_TEXT) { err = w + ": more than 2^31-1 text bytes in one call"; return -1; }      // (before the text is looked at)
    return 0;
}

int read_text_bins(Table &M, Table &P, const char *text, int64_t n, int eof, int format, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status,
                   int64_t *bad_record, double *seconds, std::string &err) {
    if (read_text_check(M, P, n, format, thre_mat, thre_pat, used, n_records, status, bad_record, seconds, err)) return -1;
    if (n > 0 && !text) { err = std::string(RT_WHAT) + ": null text"; return -1; }
    if (n > 0) {
        HIPCHK(hipSetDevice(M.device));
        uint8_t *d_text = (uint8_t *)M.workspace(Table::WS_READTEXT, (size_t)n + RT_PAD, err);
        if (!d_text) return -1;
        HIPCHK(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, M.stream));
    }
    return read_text_core(M, P, n, eof, format, n > 0 && text[n - 1] == '\n' ? 1 : 0, thre_mat, thre_pat, used, n_records, status, bad_record, seconds, err);
}

int read_text_core(Table &M, Table &P, int64_t n, int eof, int format, int last_is_lf, uint32_t thre_mat, uint32_t thre_pat, int64_t *used, int64_t *n_records, int *status,
                   int64_t *bad_record, double *seconds, std::string &err) {
    const std::string w(RT_WHAT);
    if (n < 0 || n > RT_MAX_TEXT || (format != RT_FASTQ && format != RT_FASTA)) { err = w + ": bad arguments"; return -1; }      // (read_text_check is the caller's)
    auto nothing = [&]() { M.text_records = 0; M.text_seq_bytes = 0; M.text_used = 0; return 0; };
    if (n == 0) return nothing();
    HIPCHK(hipSetDevice(M.device));
    hipStream_t st = M.stream;
    const uint64_t un = (uint64_t)n, nblk = rt_blocks(un);
    const int W = Table::WS_READTEXT;
    uint8_t *d_text = (uint8_t *)M.workspace(W, (size_t)un + RT_PAD, err);      // (the caller's: large enough, so the same buffer)
    uint64_t *d_blk = (uint64_t *)M.workspace(W + 1, (size_t)(nblk + 1) * sizeof(uint64_t), err);
    unsigned long long *d_ctl = (unsigned long long *)M.workspace(W + 9, RTC_WORDS * sizeof(unsigned long long), err);
    if (!d_text || !d_blk || !d_ctl) return -1;
    Events ev_a, ev_b, ev_c;                            // index + pack is timed in three stretches: the host sizes buffers in between
    if (ev_a.create(err) || ev_b.create(err) || ev_c.create(err)) return -1;
    double index_seconds = 0;

    // the lines
    HIPCHK(hipEventRecord(ev_a.e[0], st));
    hipLaunchKernelGGL(rt_count_lf_kernel, dim3((unsigned)nblk), dim3(RT_THREADS), 0, st, d_text, un, d_blk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_scan_tops_kernel, dim3(1), dim3(RT_SCAN_PASS), 0, st, d_blk, nblk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_a.e[1], st));
    uint64_t n_lf = 0;
    HIPCHK(hipMemcpyAsync(&n_lf, d_blk + nblk, sizeof n_lf, hipMemcpyDeviceToHost, st));
    uint8_t last_byte = 0;
    if (last_is_lf < 0) HIPCHK(hipMemcpyAsync(&last_byte, d_text + un - 1, 1, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    if (ev_a.add_seconds(index_seconds, err)) return -1;
    const TextLines T = text_lines(format, eof != 0, un, n_lf, last_is_lf < 0 ? last_byte == '\n' : last_is_lf != 0);
    if (T.ends_inside) {                                // (the host parser's first verdict, before any record is looked at)
        *status = RT_MALFORMED;
        *n_records = *bad_record = (int64_t)T.fastq_records;
        if (seconds) seconds[0] = index_seconds;
        return 0;
    }
    if (T.nl_use == 0) {
        if (seconds) seconds[0] = index_seconds;
        return nothing();
    }
    const TextBuffers B = text_buffers(un, T);
    const uint64_t nl = T.nl_use, nlb = rt_blocks(nl);
    uint32_t *d_nlpos = (uint32_t *)M.workspace(W + 2, B.nlpos, err);
    uint64_t *d_val = (uint64_t *)M.workspace(W + 3, B.line_words, err);
    uint64_t *d_pre = (uint64_t *)M.workspace(W + 4, B.line_words, err);
    uint64_t *d_lblk = (uint64_t *)M.workspace(W + 5, B.line_blocks, err);
    if (!d_nlpos || !d_val || !d_pre || !d_lblk) return -1;
    HIPCHK(hipEventRecord(ev_b.e[0], st));
    HIPCHK(hipMemsetAsync(d_ctl, 0xFF, sizeof(unsigned long long), st));      // (no bad record)
    hipLaunchKernelGGL(rt_nlpos_kernel, dim3((unsigned)nblk), dim3(RT_THREADS), 0, st, d_text, un, d_blk, T.virtual_end ? (uint32_t)n_lf : 0xFFFFFFFFu, d_nlpos);
    HIPCHK(hipGetLastError());
    const unsigned line_grid = (unsigned)((nl + RT_THREADS - 1) / RT_THREADS);
    hipLaunchKernelGGL(rt_lines_kernel, dim3(line_grid), dim3(RT_THREADS), 0, st, d_text, d_nlpos, (uint32_t)nl, format, d_val, d_ctl);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_scan_reduce_kernel, dim3((unsigned)nlb), dim3(RT_THREADS), 0, st, d_val, nl, d_lblk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_scan_tops_kernel, dim3(1), dim3(RT_SCAN_PASS), 0, st, d_lblk, nlb);
    HIPCHK(hipGetLastError());
    // (nl + 1 entries: where nl fills its blocks, the total is a block of its own, whose base the scan of the totals has left behind them)
    hipLaunchKernelGGL(rt_scan_apply_kernel, dim3((unsigned)rt_blocks(nl + 1)), dim3(RT_THREADS), 0, st, d_val, nl, d_lblk, d_pre);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_b.e[1], st));
    uint64_t total = 0;
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&total, d_pre + nl, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bad, d_ctl + RTC_BAD, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    if (ev_b.add_seconds(index_seconds, err)) return -1;
    if (seconds) seconds[0] = index_seconds;
    int64_t n_rec;
    if (format == RT_FASTQ) {
        n_rec = (int64_t)T.fastq_records;
        if (bad != ~0ull) {
            *status = RT_MALFORMED;
            *n_records = n_rec;
            *bad_record = (int64_t)bad;
            return 0;
        }
    } else {
        n_rec = (int64_t)(total >> 32) - (eof ? 0 : 1);      // (without the file's end the last record's end is not known)
        if (n_rec <= 0) return nothing();
    }
    const uint64_t seq_room = total & 0xFFFFFFFFull;    // (FASTA without the file's end: the left record's bytes are in it and are not written)
    int64_t *d_rec = (int64_t *)M.workspace(W + 7, record_words((uint64_t)n_rec) * sizeof(int64_t), err);
    int64_t *d_offs = (int64_t *)M.workspace(W + 8, offset_words((uint64_t)n_rec) * sizeof(int64_t), err);
    uint8_t *d_seq = (uint8_t *)M.workspace(W + 6, (size_t)seq_room + RT_PAD, err);
    if (!d_rec || !d_offs || !d_seq) return -1;
    const int tail_at_end = format == RT_FASTQ || eof;
    HIPCHK(hipEventRecord(ev_c.e[0], st));
    hipLaunchKernelGGL(rt_records_kernel, dim3(line_grid), dim3(RT_THREADS), 0, st, d_text, un, d_nlpos, (uint32_t)nl, format, tail_at_end, d_val, d_pre, (uint64_t)n_rec, d_rec,
                       d_offs, d_ctl);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_pack_kernel, dim3((unsigned)nblk), dim3(RT_THREADS), 0, st, d_text, un, d_blk, d_nlpos, format, d_val, d_pre, d_ctl, d_seq);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_lens_kernel, dim3((unsigned)(((uint64_t)n_rec + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, st, d_offs, (uint64_t)n_rec,
                       d_rec + 2 * n_rec + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_c.e[1], st));
    unsigned long long tail[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(tail, d_ctl + RTC_USED, sizeof tail, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    if (ev_c.add_seconds(index_seconds, err)) return -1;
    if (seconds) seconds[0] = index_seconds;
    const int64_t L = (int64_t)tail[1];
    if (tail[0] > un || (uint64_t)L > seq_room) { err = w + ": the record kernels left an impossible tail"; return -1; }

    // the bins
    Events ev;
    uint32_t *d_cnt = nullptr;
    if (read_bins_core(M, P, n_rec, d_seq, nullptr, d_offs, L, thre_mat, thre_pat, ev, &d_cnt, err)) return -1;
    HIPCHK(jk_stream_wait(st));
    double s = 0;
    if (ev.add_seconds(s, err)) return -1;
    if (seconds) seconds[1] = s;
    *used = (int64_t)tail[0];
    *n_records = n_rec;
    M.text_records = n_rec;
    M.text_seq_bytes = L;
    M.text_used = (int64_t)tail[0];
    return 0;
}

int rt_scan_words(hipStream_t st, const uint64_t *d_in, uint64_t n, uint64_t *d_blk, uint64_t *d_out, std::string &err) {
    const uint64_t nb = rt_blocks(n);
    if (nb) {
        hipLaunchKernelGGL(rt_scan_reduce_kernel, dim3((unsigned)nb), dim3(RT_THREADS), 0, st, d_in, n, d_blk);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(rt_scan_tops_kernel, dim3(1), dim3(RT_SCAN_PASS), 0, st, d_blk, nb);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rt_scan_apply_kernel, dim3((unsigned)rt_blocks(n + 1)), dim3(RT_THREADS), 0, st, d_in, n, d_blk, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int read_text_fetch(Table &M, int64_t n_records, int64_t *rec_start, int64_t *head_end, int64_t *lens, uint32_t *out_mat, uint32_t *out_pat, uint8_t *out_seq, std::string &err) {
    const std::string w("read text fetch");
    if (M.text_records < 0) { err = w + ": no read-text call has left anything to fetch"; return -1; }
    if (n_records != M.text_records) { err = w + ": n_records is not what the read-text call returned"; return -1; }
    if (!rec_start || (n_records && (!head_end || !lens || !out_mat || !out_pat))) { err = w + ": bad arguments"; return -1; }
    if (n_records == 0) {
        rec_start[0] = 0;
        return 0;
    }
    HIPCHK(hipSetDevice(M.device));
    hipStream_t st = M.stream;
    const size_t n = (size_t)n_records;
    const int W = Table::WS_READTEXT;
    const int64_t *d_rec = (const int64_t *)M.ws[W + 7].p;
    const uint32_t *d_cnt = (const uint32_t *)M.ws[Table::WS_READBINS + 1].p;
    HIPCHK(hipMemcpyAsync(rec_start, d_rec, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(head_end, d_rec + n + 1, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(lens, d_rec + 2 * n + 1, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_mat, d_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_pat, d_cnt + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_seq && M.text_seq_bytes) HIPCHK(hipMemcpyAsync(out_seq, M.ws[W + 6].p, (size_t)M.text_seq_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(jk_stream_wait(st));
    return 0;
}

}  // namespace jk
