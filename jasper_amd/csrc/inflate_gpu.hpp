// inflate_gpu.hpp -- ONE gzip stream inflated on the GPU (the device counterpart of pgunzip.hpp's ParallelGunzip).
//
// The host maps the file and does bookkeeping only; kernels for gfx950 (inflate_gpu.hip) decode the deflate data.  The file is
// processed in SLABS of compressed bytes.  Per slab:
//   1. gzd_find_starts_kernel: a nominal cut every `chunk` compressed bytes; one workgroup per cut tests the bit offsets after it
//      and keeps the smallest one where a dynamic-Huffman block header (the checks of ParallelGunzip::dynamic_header_at) or a gzip
//      member header starts.  The slab's first chunk is not searched: it starts where the previous slab's text ended.
//   2. gzd_decode_kernel: one decoder (one wave) per candidate start; output is u16 symbols, 0-255 a byte, 256 + p byte p of the
//      unknown 32 KB before the chunk (the symbolic form of pgunzip.hpp's two-dictionary trick).  A decoder stops at the first block
//      boundary that IS a later candidate's start (so it runs past a false candidate), or past the slab's nominal end.
//   3. host stitch: the chain of chunks from the slab's first one, each starting where the one before ended; a decoder that gave
//      up (its output arena full, its input buffer ended) leaves a GAP, inflated from there to the slab's end by zlib on the host.
//   4. gzd_window_kernel: one workgroup walks the accepted chunks in order and writes the resolved 32 KB before each.
//   5. gzd_resolve_kernel + gzd_crc_kernel: final bytes in stitched order, CRC-32 per piece (split at member ends); the host
//      combines the pieces per member and checks CRC and ISIZE against each trailer as zlib does.
// Every dependency between chunks crosses a kernel boundary on one stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace jk {

// stats[6] of jasper_inflate_file_device / jasper_last_inflate
enum { GZS_DECODERS = 0, GZS_ACCEPTED, GZS_DEVICE_BYTES, GZS_HOST_BYTES, GZS_SLABS, GZS_MEMBERS, GZS_N };

struct GzdConfig {
    size_t chunk = 32u << 10;    // compressed bytes per decoder (JASPER_INGEST_GZ_DEVICE_CHUNK)
    size_t slab = 64u << 20;     // compressed bytes per slab (device buffers: ~49x that)
    bool false_starts = false;   // test hook: one bogus candidate start inside every chunk (JASPER_INGEST_GZ_DEVICE_FALSE_STARTS=1)
    static GzdConfig from_env();
};

class DeviceGunzip {
  public:
    static constexpr int N_SLOTS = 5;           // device buffers: compressed slab, symbol arena, text, windows, small records
    using Alloc = std::function<void *(int slot, size_t bytes)>;   // nullptr: not available
    // device buffer `slot` for a file of `file_bytes` compressed bytes (every slab of it fits)
    static size_t bytes_needed(int slot, size_t file_bytes, const GzdConfig &cfg);

    DeviceGunzip(const char *path, int device, hipStream_t stream, const GzdConfig &cfg, uint64_t *stats);
    ~DeviceGunzip();
    DeviceGunzip(const DeviceGunzip &) = delete;
    DeviceGunzip &operator=(const DeviceGunzip &) = delete;
    // false when the file is not for this reader (not a regular gzip file with a valid first header, no device buffers): the
    // caller reads it the ordinary way
    bool open(const Alloc &alloc);
    // the contract of GzAhead::read: up to `want` bytes of text in order (copied device-to-host straight into dst), 0 at the
    // end, -1 on error (message in err).  Sets its device itself (it may be called from a read-ahead thread).
    long read(char *dst, size_t want);
    // read's contract with the destination in HBM on the same device: a slab's device text is copied device-to-device on the stream, a
    // gap the host has filled host-to-device.  The copies are ordered on the stream; what the host copy reads has left when this returns.
    long read_device(uint8_t *d_dst, size_t want);
    // nothing is left to hand out: the stream has ended and every byte of its text has been read
    bool at_end() const { return eof_ && dev_text_at_ >= dev_text_n_ && host_text_at_ >= host_text_.size(); }
    std::string err;

  private:
    bool next_slab();
    bool host_fill(uint64_t start_bit, uint64_t stop_bit, std::vector<uint8_t> &out, uint64_t &end_bit, bool &eof);
    bool member_end(uint32_t crc, uint32_t isize);
    void keep_window(const uint8_t *p, size_t n);

    std::string path_;
    int device_;
    hipStream_t stream_;
    GzdConfig cfg_;
    uint64_t *stats_;
    int fd_ = -1;
    const uint8_t *data_ = nullptr;
    size_t n_ = 0;
    // device buffers
    uint8_t *d_in_ = nullptr, *d_text_ = nullptr, *d_wins_ = nullptr, *d_small_ = nullptr;
    uint16_t *d_arena_ = nullptr;
    size_t in_cap_ = 0, cap_ = 0, n_dec_max_ = 0, ncuts_max_ = 0, text_cap_ = 0, pieces_max_ = 0;
    // stream state
    uint64_t cur_bit_ = 0;        // where the accepted text ends (a block start)
    bool eof_ = false;
    uint32_t crc_ = 0;            // CRC-32 and length of the current member's text so far
    uint64_t member_len_ = 0;
    size_t win_valid_ = 0;        // bytes of the window that belong to the current member (a reference before them is an error)
    std::vector<uint8_t> win_;    // the last 32 KB of text (host copy, when a gap was filled on the host)
    // text of the current slab not yet handed out
    uint64_t dev_text_n_ = 0, dev_text_at_ = 0;
    std::vector<uint8_t> host_text_;
    size_t host_text_at_ = 0;
};

}  // namespace jk
