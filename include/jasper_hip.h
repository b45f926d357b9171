/*
 * jasper_hip.h -- C-ABI of libjasper_hip.so, the MI355X-native replacement for the hot path of
 * alguoo314/JASPER:   reads -> canonical k-mer counts (HBM table) -> histogram -> scan / lookup / fix -> (bad,total).
 *
 * Plain C, opaque handles, caller-owned outputs, no exceptions, no torch types.  Every entry point returns
 * 0 on success and a negative code on failure; jasper_last_error() then returns a message (thread-local).
 * A handle may be used from one host thread at a time; all work of a handle is issued on its own HIP stream
 * of its own device.
 *
 * What each entry point replaces in the reference ("src/..." = /root/reference/src, "JF::..." = inside the
 * vendored jellyfish-2.3.0.tar.gz):
 *
 *   jasper_table_create / _destroy     `jellyfish count -s SIZE -m K` table set-up          JF::sub_commands/count_main.cc:258-283
 *                                      and jf.QueryMerFile(path) open / close               JF::swig/mer_file.i:18-36
 *   jasper_count_reads_files           `zcat -f READS | jellyfish count -C -m K /dev/stdin` src/jasper.sh:177
 *   jasper_count_reads_text            the same on an in-memory FASTA/FASTQ stream          JF::include/jellyfish/mer_overlap_sequence_parser.hpp:120-307
 *   jasper_count_bases[_device]        mer_counter_base::start hot loop on parsed bases     JF::sub_commands/count_main.cc:152-184
 *   jasper_histogram                   `jellyfish histo`                                    JF::sub_commands/histo_main.cc:34-44,64-84 (src/jasper.sh:177,189)
 *   jasper_lookup                      qf[jf.MerDNA(s).get_canonical()]                     JF::swig/mer_file.i:41, JF::swig/mer_dna.i:12-19 (src/jasper.py:70-71 ...)
 *   jasper_table_export/_import[_device]  `jellyfish merge` (sum by key)                    JF::jellyfish/merge_files.cc:44-176 -> multi-GPU table merge
 *   jasper_polish_batch + jasper_result_*   one `jasper.py --db DB --query BATCH ...` process   src/jasper.py:12-137 (invoked at src/jasper.sh:207-212)
 *   jasper_asm_*                       the perl one-liners around it: batch size, split, join        src/jasper.sh:132,155-156,220; src/jasper.py:120-128
 */
#ifndef JASPER_HIP_H
#define JASPER_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jasper_table jasper_table;
typedef struct jasper_result jasper_result;

/* one repair, as src/jasper.py:218-222 records it ([seqname, index, fixed_base, original]) */
typedef struct jasper_fixrec {
    int64_t index;     /* Base_coord: chunk- and pass-relative */
    uint32_t chunk;    /* position of the chunk in the batch */
    uint32_t seqno;    /* emission order inside (chunk, pass) */
    uint8_t pass;
    uint8_t kind;      /* 's' substitution  'i' inserted base(s) removed  'd' deleted base(s) restored  'x' path extension */
    uint8_t newc;      /* 's': new base   'd': restored base, repeated rep times */
    uint8_t oldc;      /* 's': old base   'i': removed base, repeated rep times */
    uint32_t rep;      /* 'x': length of the replaced original segment */
    uint32_t aux_off;  /* 'x': offset of  patch ++ original segment  in the chunk's aux bytes */
    uint32_t aux_len;  /* 'x': length of the patch */
} jasper_fixrec;

#define JASPER_OK 0
#define JASPER_ERR -1           /* HIP / IO / argument error */
#define JASPER_ERR_CAPACITY -2  /* table or scratch too small (message says which) */
#define JASPER_ERR_FORMAT -3    /* "Unsupported format" / "Invalid fastq sequence" (Jellyfish's wording) */
#define JASPER_ERR_REFERENCE_EXIT -4 /* the reference itself would exit(1) on this input (src/jasper.py:221 IndexError) */

const char *jasper_last_error(void);
int jasper_device_count(int *n);
/* on != 0: the long-running calls of OTHER threads (jasper_count_reads_files, jasper_table_write_jf) return JASPER_ERR ("cancelled")
 * at their next chunk / block instead of finishing -- for a driver that exits on an error elsewhere, as src/jasper.sh:23-28 kills its
 * children (`trap abort`); on == 0 re-arms.  Process-wide. */
int jasper_request_cancel(int on);
/* free and total device memory in bytes (hipMemGetInfo): lets the driver that replaces src/jasper.sh decide whether two stages
 * that the reference runs one after the other (`tee $JF_DB` at :177, then the jasper.py processes at :207-212) fit side by side */
int jasper_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* k in [1,64]; min_slots is a size hint like `jellyfish count -s` (rounded up to a power of two; the table
 * doubles by itself when half full).  k > 26 needs at least 2^(2k-53) slots (k=37: 2^21 = 32 MiB). */
int jasper_table_create(int k, uint64_t min_slots, int device, jasper_table **out);
/* open a Jellyfish "binary/sorted" database (jasper.sh -j, or an existing mer_counts$K.jf) into a new HBM table; k comes from
 * the file header like jf.QueryMerFile(path) does (JF::swig/mer_file.i:18-36); errors use Jellyfish's wording */
int jasper_table_load_jf(const char *path, int device, jasper_table **out);
void jasper_table_destroy(jasper_table *t);
/* the table as a Jellyfish "binary/sorted" database: what `jellyfish count -o mer_counts$K.jf` leaves behind
 * (src/jasper.sh:177; format JF::include/jellyfish/file_header.hpp:26-108, binary_dumper.hpp:36-40,148-199), readable by
 * jellyfish 2.3.0 query/dump/histo, QueryMerFile and jasper_table_load_jf.  cmdline[] is recorded in the header. */
/* records [n*part/nparts, n*(part+1)/nparts) of the database only: one GPU's shard of an existing DB (dist.shard_tables
 * then routes every key to its owner) */
int jasper_table_load_jf_part(const char *path, int device, uint32_t part, uint32_t nparts, jasper_table **out);
int jasper_table_write_jf(jasper_table *t, const char *path, const char *const *cmdline, int n_cmdline);
/* test hook (host arithmetic only, no GPU): the table's bijective k-mer hash (inverse = 0) or its inverse (1) */
int jasper_debug_mix(int k, int inverse, uint64_t hi, uint64_t lo, uint64_t out2[2]);
/* distinct = keys in this table; occurrences = k-mer occurrences this table's counting calls have SCANNED.  For an owner shard
 * filled by the exchange (jasper_count_exchange_*) that is what this GPU read and sent to all owners, not the occurrences of the
 * keys the shard holds (those are the sum of its counts: jasper_histogram). */
int jasper_table_info(jasper_table *t, int *k, uint64_t *slots, uint64_t *distinct, uint64_t *occurrences);
int jasper_table_sync(jasper_table *t);
/* forget every k-mer (slots and counters zeroed in place; capacity kept) */
int jasper_table_clear(jasper_table *t);

/* bases: concatenated read sequences, records separated by any non-ACGTacgt byte; windows do not span calls */
int jasper_count_bases(jasper_table *t, const char *bases, uint64_t n);
/* the same with the bases already resident in this table's device memory (16-byte aligned for full speed) */
int jasper_count_bases_device(jasper_table *t, const void *d_bases, uint64_t n);
int jasper_count_reads_text(jasper_table *t, const char *text, uint64_t n);
int jasper_count_reads_files(jasper_table *t, const char *const *paths, int n_paths);
/* the same over a byte range [begins[i], ends[i]) of every file (ends[i] < 0: to its end) -- one GPU's shard of the reads.
 * Ranges must start at record boundaries (jasper_amd/dist.py plan_read_shards finds them); a gzip file cannot be cut: it
 * is read whole if its range starts at 0 and skipped otherwise.  Counts are sums over reads, so the shards' tables add up
 * to the table of the whole input. */
int jasper_count_reads_file_ranges(jasper_table *t, const char *const *paths, const int64_t *begins, const int64_t *ends, int n_paths);

/* of the last jasper_count_reads_files call: text bytes parsed by the GPU kernels / by the host state machine (the
 * fallback for multi-line records, DOS line ends, malformed input and stream tails) */
int jasper_last_ingest(jasper_table *t, uint64_t *gpu_bytes, uint64_t *host_bytes);
/* of the last jasper_count_reads_files* or feed call: the gzip input, summed over its files --
 *   stats[0] decoders launched by the device inflater, [1] chunks it accepted into the text, [2] text bytes inflated on the device,
 *   [3] text bytes inflated on the host (zlib or the many-thread reader: files not selected for the device, spans it gave back),
 *   [4] slabs, [5] gzip members checked by the device inflater.
 * A regular gzip file read from byte 0 goes to the device inflater when it has at least JASPER_INGEST_GZ_DEVICE_MIN_MB compressed
 * MiB (JASPER_INGEST_GZ=auto, the default; with that variable unset, never), always (=device) or never (=host). */
int jasper_last_inflate(jasper_table *t, uint64_t stats[6]);
int jasper_histogram(jasper_table *t, uint64_t *out10002);
/* the same over the keys of ONE owner partition (as in jasper_table_export_packed): after a multi-GPU merge every rank
 * bins the range it owns and the 10002 bins are summed over ranks, instead of every rank scanning the whole table */
int jasper_histogram_part(jasper_table *t, uint32_t part, uint32_t nparts, uint64_t *out10002);
/* 1 if the histogram is already known because the last counting call binned the final counts while it wrote them
 * (one partitioned pass over the whole input into an empty table); jasper_histogram then costs one small copy */
int jasper_histogram_is_fused(jasper_table *t);
/* string i is chars[offsets[i] .. offsets[i+1]); out[i] = count of canonical(pad(string i)) clamped to 2^32-1 */
int jasper_lookup(jasper_table *t, const char *chars, const int64_t *offsets, uint64_t n, uint32_t *out);

/* entries are 3 x uint64 each: mixed-hash high word, low word, exact count.  Any table with the same k accepts them. */
int jasper_table_export(jasper_table *t, uint64_t *n_entries, uint64_t *host_entries /* NULL: size query */);
int jasper_table_import(jasper_table *t, const uint64_t *host_entries, uint64_t n_entries);
int jasper_table_export_device(jasper_table *t, uint64_t *n_entries, void **d_entries);
int jasper_table_import_device(jasper_table *t, const void *d_entries, uint64_t n_entries);
/* export into caller-owned device memory (e.g. a torch tensor handed to RCCL); cap_entries = room in d_dst */
int jasper_table_export_to(jasper_table *t, void *d_dst, uint64_t cap_entries, uint64_t *n_entries);
int jasper_device_free(jasper_table *t, void *d_ptr);
/* multi-GPU exchange format: 16-byte entries { hash.lo, hash.hi | count << max(0, 2k-64) } in device memory.
 * export: keys whose home slot lies in slot-range partition `part` of `nparts` (nparts = 1: all); *n_entries is the
 * number that exists (may exceed cap_entries: call once with cap 0 to size the buffer).  import mode 0 adds the
 * counts (key-wise sum), mode 1 sets them (an owner's final counts replace this table's partial ones). */
int jasper_table_export_packed(jasper_table *t, void *d_dst, uint64_t cap_entries, uint64_t *n_entries, uint32_t part, uint32_t nparts);
int jasper_table_import_packed(jasper_table *t, const void *d_src, uint64_t n_entries, int mode);
/* add up to 8 entry lists in ONE sweep over the table (an owner adding what every rank sent it): the lists are in slot order
 * of same-hash tables, so their c-th parts land in the same band of slots, which stays in cache while all lists update it */
int jasper_table_import_packed_multi(jasper_table *t, const void *const *d_srcs, const uint64_t *counts, uint32_t n_src);
/* grow to at least min_slots slots (ranks agree on one geometry before exchanging slot-range partitions) */
int jasper_table_reserve(jasper_table *t, uint64_t min_slots);
/* rehash into the smallest slot count that holds the present keys at a load of at most max_load (0.05 .. 0.9); may shrink */
int jasper_table_fit(jasper_table *t, double max_load);

/* Owner-sharded table ("keep the table key-sharded and route lookups").  Instead of replicating the merged
 * table on every GPU, owner o of n keeps ONLY the keys with jasper_owner_of(hash) == o, and every lookup -- the polishing
 * kernels', jasper_lookup's -- reads the owner's slot array directly: its own HBM, or a peer's over xGMI.
 *   jasper_table_export_owner: all entries of t in the exchange format above, grouped by owner; segment o starts at
 *     d_dst + o * cap_entries * 16 bytes and holds counts[o] entries (if any counts[o] > cap_entries nothing beyond cap was
 *     written: call again with more room).  One pass over the table whatever n_owners is.
 *   jasper_table_ipc_handle: 64 bytes that let another PROCESS map this table's slot array (hipIpcGetMemHandle).
 *   jasper_table_attach_ipc: handles = n x 64 bytes in owner order (entry `self` unused).  All owners' tables must have
 *     the geometry of t (same k, same slot count: jasper_table_reserve after agreeing on the maximum).
 *   jasper_table_attach_tables: the same for shard tables living in this process.
 *   jasper_table_detach: back to a whole table.  Growing a table detaches it.
 * The owners' tables must not be written while any GPU reads them; that ordering is the caller's (a barrier). */
int jasper_table_export_owner(jasper_table *t, void *d_dst, uint64_t cap_entries, uint32_t n_owners, uint64_t *counts);
/* The read files as a FEED of base batches in HBM (role of `zcat -f $READS |` in front of a counter that is driven from outside,
 * src/jasper.sh:177): the reader / inflater / parsers of jasper_count_reads_file_ranges run in a thread of their own, but every
 * batch of bases they would have counted into t is handed to the caller instead.  `t` only lends its device and buffers (its
 * table is not touched).  begins / ends: per-file byte ranges as for jasper_count_reads_file_ranges, or both NULL.
 *   jasper_read_feed_next     waits for the next batch: *d_bases (text bases with a non-base byte between records, as
 *                             jasper_count_bases_device takes them; no k-mer spans two batches), *n bytes.  *n == 0: the stream
 *                             has ended and the feed is closed; a reader / parser error is returned here.
 *   jasper_read_feed_release  the caller is done with the batch: its memory is reused for the next one. */
int jasper_read_feed_start(jasper_table *t, const char *const *paths, const int64_t *begins, const int64_t *ends, int n_paths);
int jasper_read_feed_next(jasper_table *t, const void **d_bases, uint64_t *n);
int jasper_read_feed_release(jasper_table *t);
/* Counting on several GPUs WITHOUT per-GPU tables that are merged afterwards (role of `jellyfish count` over all reads,
 * src/jasper.sh:177, and of JF::jellyfish/merge_files.cc:44-96): the reads of every GPU go through the two partition passes
 * of the atomic-free counting path; the second pass also groups by owner, so what owner o is to receive is one contiguous
 * block of the send buffers -- the region lists of o's own table.  After ONE all_to_all of those blocks (8 bytes per k-mer
 * occurrence plus the slack of the lists) every owner inserts what it received straight into its shard `t`.  All ranks call
 * with shard tables of one geometry and the same piece_max (the longest piece [pos, end) any of them scans in this round)
 * and records_max (the most records any rank's scan returned; 0 = not known, piece_max stands in: the lists, and with them
 * the bytes that travel, are then sized for the worst case).
 *   jasper_count_exchange_plan      out8 = { records (8 B) per owner block, slice counts (4 B) per owner block, deferred entries
 *                                   (24 B) to provide room for, p1, p2 (+ 256 x the second-level bits left to an extra pass
 *                                   on the owner: very large shards), region bits, slices per list, slice capacity };
 *                                   returns 1 (not an error) when this table / piece size / k has no such geometry: count into a
 *                                   table per GPU and use jasper_table_export_owner instead.
 *   jasper_count_exchange_scan      first pass over bases [pos, end) of d_bases (n bytes, text bases as for
 *                                   jasper_count_bases_device; the k-1 bases before pos are read as context) into lists kept
 *                                   inside t; *records = k-mer occurrences found.  d_deferred: 64-byte header (word 0 =
 *                                   entries), then entries of 3 words hash.hi, hash.lo, increment -- the few records that found
 *                                   no room in their list, here or in the next call.  Returns when the pass is done.
 *   jasper_count_exchange_partition second pass: the lists of the scan -> d_send (n_owners blocks of records), d_send_counts
 *                                   (n_owners blocks of counts); asynchronous like the counting calls (jasper_table_sync).
 *   jasper_count_exchange_dedupe    optional, between partition and the all_to_all: every list of d_send is deduplicated in
 *                                   place -- one record per distinct key, (occurrences - 1) in *count_bits of the record's bits
 *                                   that its list implies -- the counts are updated and *max_fill = records in the fullest
 *                                   list: only that many per list need to travel (the caller packs [list][slice capacity] to
 *                                   [list][max over ranks of max_fill]).  Returns 1 (not an error, nothing done) when the
 *                                   geometry has no such bits.  Returns when the pass is done.
 *   jasper_count_exchange_insert    d_recv / d_recv_counts: block s = what rank s put into its block `self`; d_deferred_all: the
 *                                   deferred entries of ALL ranks back to back (the ones owned by `self` are added);
 *                                   whole_input != 0: these lists are all that goes into the (empty) shard, so the multiplicity
 *                                   histogram is taken on the way (jasper_histogram_is_fused).  slice_cap / count_bits: 0, or the
 *                                   packed slice capacity and the count bits after jasper_count_exchange_dedupe. */
int jasper_count_exchange_plan(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, uint64_t *out8);
int jasper_count_exchange_scan(jasper_table *t, const void *d_bases, uint64_t n, uint64_t pos, uint64_t end, uint64_t piece_max, uint32_t n_owners, void *d_deferred,
                               uint64_t deferred_cap, uint64_t *records);
int jasper_count_exchange_partition(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, void *d_send, void *d_send_counts, void *d_deferred,
                                    uint64_t deferred_cap);
int jasper_count_exchange_dedupe(jasper_table *t, uint64_t piece_max, uint64_t records_max, uint32_t n_owners, void *d_send, void *d_send_counts, uint32_t *max_fill,
                                 int *count_bits);
int jasper_count_exchange_insert(jasper_table *t, const void *d_recv, const void *d_recv_counts, uint64_t piece_max, uint64_t records_max, uint32_t n_owners,
                                 uint32_t self, const void *d_deferred_all, uint64_t n_deferred_all, int whole_input, uint32_t slice_cap, int count_bits);
/* A binary/sorted database written by several GPUs: the file order (pos, key) with `size` = 2^size_log2 is the numeric order
 * of the key rotated right by size_log2 bits, so cutting the value range of the key's low size_log2 bits into n_ranges equal
 * parts cuts the file into n_ranges consecutive pieces.  jasper_table_export_file_ranges groups the entries of t by that
 * range (same layout and conventions as jasper_table_export_owner); after an all_to_all each GPU holds one range, sorts it
 * and writes it with jasper_table_write_jf_piece (what = 1: records only; 2: the header only; 0: both). */
int jasper_table_export_file_ranges(jasper_table *t, void *d_dst, uint64_t cap_entries, uint32_t n_ranges, int size_log2, uint64_t *counts);
int jasper_table_write_jf_piece(jasper_table *t, const char *path, const char *const *cmdline, int n_cmdline, int size_log2, int what);
int jasper_table_ipc_handle(jasper_table *t, void *out64);
int jasper_table_attach_ipc(jasper_table *t, const void *handles, uint32_t n, uint32_t self);
int jasper_table_attach_tables(jasper_table *t, jasper_table *const *shards, uint32_t n, uint32_t self);
int jasper_table_detach(jasper_table *t);
/* open and close the peers' handles without a table: run from a throw-away process with a time limit before the real
 * attach (jasper_amd/dist.py), so that a mapping call that never returns costs a killed helper, not a hung GPU process */
int jasper_ipc_probe(int device, const void *handles, uint32_t n, uint32_t self);
/* owner of a packed entry's hash among n (host-side restatement of the device function, for tests and routing) */
uint32_t jasper_owner_of(uint64_t hash_lo, uint64_t hash_hi, uint32_t n);

/* one batch of chunk records through `passes` fixing passes + the final QV pass (src/jasper.py:25-26) */
int jasper_polish_batch(jasper_table *t, int n_chunks, const char *const *seqs, const int64_t *lens,
                        int solid_thre, int passes, int fix, jasper_result **out);
/* the same with the chunk records already in HBM on the table's device (chunk c = d_text[offsets[c] .. offsets[c+1]),
 * offsets is a host array of n_chunks+1 entries).  The polished text is left in HBM: jasper_result_seq_device points at
 * it, jasper_result_seq copies it to the host on first use.  It lies in the table's workspace, so the library copies it
 * to the host by itself before the next polish call on the same table (or jasper_table_destroy) would overwrite it;
 * after that jasper_result_seq_device fails and jasper_result_seq still works. */
int jasper_polish_batch_device(jasper_table *t, int n_chunks, const void *d_text, const int64_t *offsets,
                               int solid_thre, int passes, int fix, jasper_result **out);
int jasper_result_num_chunks(const jasper_result *r);
int jasper_result_seq(const jasper_result *r, int chunk, const char **seq, int64_t *len);
int jasper_result_seq_len(const jasper_result *r, int chunk, int64_t *len);
int jasper_result_seq_device(const jasper_result *r, int chunk, const void **d_seq, int64_t *len);
int jasper_result_records(const jasper_result *r, const jasper_fixrec **recs, uint64_t *n);
int jasper_result_aux(const jasper_result *r, int chunk, const char **aux, uint64_t *n);
int jasper_result_qv(const jasper_result *r, int64_t out4[4]); /* bad0,total0,badP,totalP  (src/jasper.py:107-111) */
/* the same four counters for one chunk record (a caller that polishes several batch files in one call splits them again) */
int jasper_result_qv_chunk(const jasper_result *r, int chunk, int64_t out4[4]);
int jasper_result_lookups(const jasper_result *r, uint64_t *n);
double jasper_result_seconds(const jasper_result *r);         /* device time of the passes (HIP events) */
/* how the batch was parallelised: segments walked over all passes, chunks redone unsegmented after a failed speculation */
int jasper_result_segments(const jasper_result *r, uint64_t *n_segments, uint64_t *n_respeculated);
/* where a pass may cut a chunk of a table of this k into segments (no GPU call; tests restate the rule from these):
 * out5 = TMIN (least distance between sync points, and from the last one to the chunk end), CMIN (least distance between a
 * clean-zone boundary and its neighbours), CLEAN_CELL (one boundary candidate per this many positions), W (clean windows
 * required left of a sync point), M (text a segment keeps right of the next sync point) */
int jasper_polish_cut_geometry(int k, int64_t out5[5]);
/* 1 if the batch had to be repeated with larger internal buffers (results are the same either way) */
int jasper_result_retried(const jasper_result *r);
void jasper_result_free(jasper_result *r);

/* Dense k-mer report: per-sequence counters and the maximal runs of unreliable k-mers, computed on the GPU from the resident
 * table (whole or attached owner-sharded, any k <= 64).
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  Its QV pass (src/jasper.py:50-111) walks the
 * chunk records with a stride and prints two numbers for the whole assembly (src/jasper.sh:239-242); that stays what it is
 * (jasper_result_qv).  What it is: the windows of src/jasper.py:55-71 taken DENSELY over whole sequences, to be turned into a QV
 * per sequence by the formula of src/jasper.sh:239-242.  For a sequence of n bytes and the table's k:
 *   window i (0 <= i <= n-k)  valid       iff all its k bytes are ACGTacgt (case folded)
 *                             count       the table's count of its canonical k-mer, clamped to 2^32-1 as jasper_lookup does
 *                             unreliable  valid and count < thre        (thre == 0: none)
 *                             absent      valid and count == 0          (counted whether or not it is unreliable too)
 *   run                       a maximal range of consecutive unreliable windows of one sequence (an invalid or reliable window,
 *                             or the sequence's end, ends it): first window, windows, absent windows among them, smallest count
 * Sequences shorter than k (empty ones too) are legal and give zeros.  Runs are ordered by (seq, start).  The table is not
 * modified.  The library sizes its buffers by itself and repeats the scan when there are more runs than it had room for
 * (jasper_report_retried), so a call succeeds whatever the input is.  The kernel works in tiles of
 * jasper_report_tile_windows() = 4096 windows of one sequence; runs are stitched across tiles.
 *   jasper_kmer_report         sequences in host memory
 *   jasper_kmer_report_device  sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the table's device; offsets is a host
 *                              array of n_seqs+1 entries
 *   jasper_report_counts       out4 = windows, valid, unreliable, absent of one sequence
 *   jasper_report_runs         the run list (owned by the report)
 *   jasper_report_seconds      device time of the report's kernels (HIP events) */
typedef struct jasper_report jasper_report;
typedef struct jasper_kmer_run { int64_t start; uint64_t n_kmers; uint64_t n_absent; uint32_t seq; uint32_t min_count; } jasper_kmer_run;
int jasper_kmer_report(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_report **out);
int jasper_kmer_report_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, jasper_report **out);
int jasper_report_tile_windows(void);
int jasper_report_num_seqs(const jasper_report *r);
int jasper_report_counts(const jasper_report *r, int seq, uint64_t out4[4]);   /* windows, valid, unreliable, absent */
int jasper_report_runs(const jasper_report *r, const jasper_kmer_run **runs, uint64_t *n);
double jasper_report_seconds(const jasper_report *r);                           /* device time, HIP events */
int jasper_report_retried(const jasper_report *r);
void jasper_report_free(jasper_report *r);

/* Copy-number k-mer spectrum: two resident tables of the same k on the same device -- `reads` (R) and `assembly` (A, the assembly's
 * contigs counted into a table of its own with the usual counting calls: case folded, every non-ACGT byte a separator) -- joined on
 * the GPU.  No key crosses to the host.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart (it is the spectra-cn / completeness half of a
 * k-mer evaluation; jasper_kmer_report is the other half).  The spectrum is a matrix S[6][10002] of unsigned 64-bit cells, row-major:
 *   row m     = min(count in A, 5): 0 = not in the assembly, 5 = five copies or more          (jasper_spectrum_rows() = 6)
 *   column c  = min(min(count in R, 2^32-1), 10001), the binning of jasper_histogram: 0 = not in the reads
 *   S[m][c], c >= 1   distinct keys of R with that (m, c)
 *   S[m][0], m >= 1   distinct keys of A that R does not have: the assembly-only k-mers by copy number
 *   S[0][0]           0
 * A slot whose count is 0 is no key, in either table (as for jasper_histogram).  So the sum over m of S[m][c] is R's histogram bin c
 * for every c >= 1, and the sum over all c of S[m][c] is A's histogram bin m for m = 1..4, bins 5.. together for m = 5.  From it,
 * for a threshold t >= 1 (jasper_amd/spectra.py): solid = sum over c >= t and all m, found = the same over m >= 1, completeness =
 * found / solid, asm_distinct = sum over m >= 1 and all c, asm_only = sum over m >= 1 of S[m][0].
 * Either table may be narrow or wide.  R may be an attached owner-sharded table (every owner's shard is swept); A must be a whole
 * table.  Neither table is modified.  A different k, different devices, an attached A, or the same handle twice is JASPER_ERR.
 * out_cells: 6 * 10002 words in host memory; device_seconds (may be NULL): device time of the two sweeps, HIP events. */
int jasper_spectrum_rows(void);
int jasper_table_spectrum(jasper_table *reads, jasper_table *assembly, uint64_t *out_cells /* 6 * 10002, row-major */, double *device_seconds);

/* Copy-number scan: WHERE on the sequences the reads support another number of copies than the assembly holds.  Two resident tables of
 * the same k on the same device -- `reads` (R, whole or attached owner-sharded) and `assembly` (A, a whole table, a different handle from
 * R; otherwise JASPER_ERR as for jasper_table_spectrum) -- and a set of sequences, scanned densely on the GPU as jasper_kmer_report
 * scans them, every window looked up in both tables.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  jasper_table_spectrum counts the distinct k-mers
 * that are collapsed or duplicated; this locates them.  `peak` (>= 1, else JASPER_ERR) is the read count of a k-mer present once in the
 * genome.  For a sequence of n bytes and the tables' k:
 *   window i (0 <= i <= n-k)  valid    iff all its k bytes are ACGTacgt (case folded)
 *                             c        R's count of its canonical k-mer, clamped to 2^32-1
 *                             a        A's count of it, clamped to 2^32-1 (0 is possible: A need not be counted from this text)
 *                             e        (2 c + peak) div (2 peak) in 64-bit arithmetic: the copies the reads support, rounded half up
 *                             excess   (class 1) valid, c >= thre and e > a: the reads support more copies than A holds -- collapsed
 *                             deficit  (class 2) valid, c >= thre and e < a: A holds more copies than the reads support -- duplicated
 *                                      or thinly supported
 *                             class 0  otherwise.  Windows with c < thre are jasper_kmer_report's business; with thre == 0 a valid
 *                                      window with c == 0 and a >= 1 is `deficit`
 *   per sequence              six counters: windows, valid, excess, deficit, sum_reads, sum_asm (the sums of c and of a over its valid
 *                             windows)
 *   run                       a maximal range of consecutive windows of one sequence with the same non-zero class (a window of another
 *                             class, an invalid window or the sequence's end ends it; an excess window directly followed by a deficit
 *                             window gives two runs that touch): first window, windows, sums of c and of a over them, sequence, class
 * Sequences shorter than k (empty ones too) are legal and give zeros.  Runs are ordered by (seq, start).  Neither table is modified and
 * the result is the same on every call.  The library sizes its run buffer by itself and repeats the scan once when there were more runs
 * than it had room for (jasper_copyrep_retried).  Tiles are those of the report (jasper_report_tile_windows()).
 *   jasper_copy_report         sequences in host memory
 *   jasper_copy_report_device  sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the tables' device; offsets is a host array of
 *                              n_seqs+1 entries
 *   jasper_copyrep_counts      out6 = windows, valid, excess, deficit, sum_reads, sum_asm of one sequence
 *   jasper_copyrep_runs        the run list (owned by the result)
 *   jasper_copyrep_seconds     device time of the scan's kernels (HIP events) */
typedef struct jasper_copyrep jasper_copyrep;
typedef struct jasper_copy_run { int64_t start; uint64_t n_kmers; uint64_t sum_reads; uint64_t sum_asm; uint32_t seq; uint32_t kind; } jasper_copy_run;
int jasper_copy_report(jasper_table *reads, jasper_table *assembly, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak,
                       jasper_copyrep **out);
int jasper_copy_report_device(jasper_table *reads, jasper_table *assembly, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak,
                              jasper_copyrep **out);
int jasper_copyrep_num_seqs(const jasper_copyrep *r);
int jasper_copyrep_counts(const jasper_copyrep *r, int seq, uint64_t out6[6]);   /* windows, valid, excess, deficit, sum_reads, sum_asm */
int jasper_copyrep_runs(const jasper_copyrep *r, const jasper_copy_run **runs, uint64_t *n);
double jasper_copyrep_seconds(const jasper_copyrep *r);                          /* device time, HIP events */
int jasper_copyrep_retried(const jasper_copyrep *r);
void jasper_copyrep_free(jasper_copyrep *r);

/* Pair spectrum: both haplotypes of a diploid assembly against the reads.  Three resident tables of the same k on the same device --
 * `reads` (R), `assembly` (A1) and `alt` (A2, the other haplotype), the latter two counted as jasper_table_spectrum's A is -- joined on the
 * GPU.  No key crosses to the host.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart (the diploid mode of a k-mer evaluation).  The
 * result is a matrix P[4][10002] of unsigned 64-bit cells, row-major:
 *   row j     = (count in A1 >= 1 ? 1 : 0) | (count in A2 >= 1 ? 2 : 0): 0 = reads only, 1 = asm only, 2 = alt only, 3 = shared
 *   column c  = min(min(count in R, 2^32-1), 10001), the binning of jasper_histogram: 0 = not in the reads
 *   P[j][c], c >= 1   distinct keys of R with that (j, c)
 *   P[j][0], j >= 1   distinct keys of A1 u A2 that R does not have, each counted once
 *   P[0][0]           0
 * A slot whose count is 0 is no key, in any of the tables.  With S1 = the spectrum of (R, A1) and S2 = that of (R, A2), for every c:
 * P[1][c] + P[3][c] = sum over m >= 1 of S1[m][c], P[2][c] + P[3][c] = the same of S2, and for c >= 1 the sum over j of P[j][c] is R's
 * histogram bin c.  Copy numbers are not kept (jasper_table_spectrum has them per assembly).
 * Any table may be narrow or wide; all three must be whole tables (an attached owner-sharded R is refused here, unlike
 * jasper_table_spectrum's).  No table is modified.  A different k, different devices, an attached table, or a handle given twice is
 * JASPER_ERR, each with its own message.
 * out_cells: 4 * 10002 words in host memory; device_seconds (may be NULL): device time of the three sweeps, HIP events. */
int jasper_table_spectrum_pair(jasper_table *reads, jasper_table *assembly, jasper_table *alt, uint64_t *out_cells /* 4 * 10002, row-major */,
                               double *device_seconds);

/* Pair scan: WHERE on one haplotype's sequences the k-mers lie that the other haplotype does not hold.  Two resident tables of the same
 * k on the same device -- `reads` (R) and `other` (O, the OTHER haplotype's sequences counted into a table of its own), both whole
 * tables and different handles (otherwise JASPER_ERR as for jasper_table_spectrum_pair) -- and a set of sequences of THIS haplotype,
 * scanned densely on the GPU as jasper_kmer_report scans them, every window looked up in both tables.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  For a sequence of n bytes and the tables' k:
 *   window i (0 <= i <= n-k)  valid          iff all its k bytes are ACGTacgt (case folded)
 *                             c              R's count of its canonical k-mer, clamped to 2^32-1
 *                             b              O's count of it
 *                             unreliable     valid and c < thre; absent: valid and c == 0 (jasper_kmer_report's rules)
 *                             private_solid  (class 1) valid, b == 0 and c >= thre: the haplotypes differ here and the reads hold this
 *                                            haplotype's allele (a SNP between the haplotypes gives a run of k windows on each)
 *                             private_weak   (class 2) valid, b == 0 and c < thre: an error only this haplotype has
 *                             class 0        otherwise; an unreliable window that is not private is an unsupported k-mer both
 *                                            haplotypes hold.  With thre == 0 nothing is unreliable and nothing is weak
 *   per sequence              six counters: windows, valid, unreliable, absent, private_solid, private_weak; the first four are
 *                             jasper_kmer_report's for the same sequences and threshold
 *   run                       a maximal range of consecutive windows of one sequence with the same non-zero class (a solid window
 *                             directly followed by a weak one gives two runs that touch): first window, windows, the sum of c over
 *                             them, sequence, class
 * Sequences shorter than k (empty ones too) are legal and give zeros.  Runs are ordered by (seq, start).  Neither table is modified and
 * the result is the same on every call.  The library sizes its run buffer by itself and repeats the scan once when there were more runs
 * than it had room for (jasper_pairscan_retried).  Tiles are those of the report (jasper_report_tile_windows()).
 *   jasper_pair_scan           sequences in host memory
 *   jasper_pairscan_counts     out6 = windows, valid, unreliable, absent, private_solid, private_weak of one sequence
 *   jasper_pairscan_runs       the run list (owned by the result)
 *   jasper_pairscan_seconds    device time of the scan's kernels (HIP events) */
typedef struct jasper_pairscan jasper_pairscan;
typedef struct jasper_pair_run { int64_t start; uint64_t n_kmers; uint64_t sum_reads; uint32_t seq; uint32_t kind; } jasper_pair_run;
int jasper_pair_scan(jasper_table *reads, jasper_table *other, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_pairscan **out);
int jasper_pairscan_num_seqs(const jasper_pairscan *r);
int jasper_pairscan_counts(const jasper_pairscan *r, int seq, uint64_t out6[6]);   /* windows, valid, unreliable, absent, private_solid, private_weak */
int jasper_pairscan_runs(const jasper_pairscan *r, const jasper_pair_run **runs, uint64_t *n);
double jasper_pairscan_seconds(const jasper_pairscan *r);                          /* device time, HIP events */
int jasper_pairscan_retried(const jasper_pairscan *r);
void jasper_pairscan_free(jasper_pairscan *r);

/* Trio hap-mer scan and census: WHERE on the sequences the k-mers lie that only one parent's reads hold, and how many of them an assembly
 * has.  The tables, all of the same k on the same device and all different handles:
 *   mat (M), pat (P)  the mother's and the father's reads, whole tables
 *   child (R)         the child's reads, whole or attached owner-sharded; may be NULL = no inheritance filter
 *   assembly (A)      census only: a whole table, the contigs counted into it; may be NULL
 * thre_mat, thre_pat and thre_child are each at least 1 (thre_child too when child is NULL).  A different k, different devices, the
 * same handle twice, an attached M, P or A, or a threshold of 0 is JASPER_ERR with a message that names the cause.  No table is modified.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart (it is the trio half of a k-mer evaluation).  A
 * hap-mer here is what Merqury's is: a k-mer of one parent whose count in the OTHER parent is exactly 0 (the difference of the two
 * parental sets), kept when it is solid in that parent and, with a child table, inherited (solid in the child).
 *
 * Scan.  For a sequence of n bytes and the tables' k:
 *   window i (0 <= i <= n-k)  valid    iff all its k bytes are ACGTacgt (case folded)
 *                             m, p, c  the counts of its canonical k-mer in M, P, R, each clamped to 2^32-1
 *                             mat      (class 1) valid, m >= thre_mat, p == 0 and (R is NULL or c >= thre_child)
 *                             pat      (class 2) valid, p >= thre_pat, m == 0 and (R is NULL or c >= thre_child)
 *                             class 0  otherwise.  No window has both classes
 *   per sequence              four counters: windows, valid, mat, pat
 *   run (= one marker)        a maximal range of consecutive windows of one sequence with the same non-zero class (a window of another
 *                             class, an invalid window or the sequence's end ends it; a mat window directly followed by a pat window
 *                             gives two runs that touch): first window, windows, sequence, class
 * Sequences shorter than k (empty ones too) are legal and give zeros.  Runs are ordered by (seq, start) and the result is the same on
 * every call.  The library sizes its run buffer by itself and repeats the scan once when there were more runs than it had room for
 * (jasper_hapscan_retried).  Tiles are those of the report (jasper_report_tile_windows()).  The kernels run on the child's stream, on
 * the mother's when child is NULL.
 *   jasper_hapmer_scan         sequences in host memory
 *   jasper_hapmer_scan_device  sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the tables' device; offsets is a host array of
 *                              n_seqs+1 entries
 *   jasper_hapscan_counts      out4 = windows, valid, mat, pat of one sequence
 *   jasper_hapscan_runs        the run list (owned by the result)
 *   jasper_hapscan_seconds     device time of the scan's kernels (HIP events)
 *
 * Census.  H_mat = the distinct keys x of M with M[x] >= thre_mat, P[x] == 0 and (R NULL or R[x] >= thre_child), counts clamped as above;
 * H_pat the same with the parents swapped.  out6 = for H_mat, then for H_pat:
 *   hapmers      |H|
 *   found        the keys of H with A[x] >= 1
 *   occurrences  the sum over H of A[x] (a 64-bit sum of the clamped counts)
 * found and occurrences are 0 when assembly is NULL.  When A was counted from exactly the scanned sequences, occurrences of mat equals the
 * scan's total of mat windows, and of pat likewise.  device_seconds (may be NULL): device time of the two sweeps, HIP events. */
typedef struct jasper_hapscan jasper_hapscan;
typedef struct jasper_hap_run { int64_t start; uint64_t n_kmers; uint32_t seq; uint32_t kind; } jasper_hap_run;
int jasper_hapmer_scan(jasper_table *mat, jasper_table *pat, jasper_table *child, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre_mat,
                       uint32_t thre_pat, uint32_t thre_child, jasper_hapscan **out);
int jasper_hapmer_scan_device(jasper_table *mat, jasper_table *pat, jasper_table *child, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre_mat,
                              uint32_t thre_pat, uint32_t thre_child, jasper_hapscan **out);
int jasper_hapscan_num_seqs(const jasper_hapscan *r);
int jasper_hapscan_counts(const jasper_hapscan *r, int seq, uint64_t out4[4]);   /* windows, valid, mat, pat */
int jasper_hapscan_runs(const jasper_hapscan *r, const jasper_hap_run **runs, uint64_t *n);
double jasper_hapscan_seconds(const jasper_hapscan *r);                          /* device time, HIP events */
int jasper_hapscan_retried(const jasper_hapscan *r);
void jasper_hapscan_free(jasper_hapscan *r);
int jasper_hapmer_census(jasper_table *mat, jasper_table *pat, jasper_table *child, jasper_table *assembly, uint32_t thre_mat, uint32_t thre_pat, uint32_t thre_child,
                         uint64_t out6[6] /* mat: hapmers, found, occurrences; then pat */, double *device_seconds);

/* A join of tables as a table: the census's set H, kept instead of counted.  src (S), absent (A) and dst are whole tables of the same k
 * on the same device, all handles different; solid (R) may be NULL and may be an attached owner-sharded table; thre_src and thre_solid
 * are each at least 1; dst holds no key.  Anything else -- a different k, different devices, the same handle twice, an attached S, A or
 * dst, a threshold of 0, a dst with keys -- is JASPER_ERR with a message that names the cause, before any table is touched.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.
 *
 * Selected = the distinct keys x of S with S[x] >= thre_src (the 64-bit count), A[x] == 0 and (R NULL or min(R[x], 2^32-1) >=
 * thre_solid).  After the call dst holds exactly the selected keys, each with its 64-bit count S[x]; S, A and R are not modified.  With
 * thre_src = the parent's threshold this is H_mat of jasper_hapmer_census(S, A, R, ...): `selected` equals its `hapmers`.
 *   out4 = candidates   keys of S with S[x] >= thre_src
 *          in_absent    candidates dropped because A holds them
 *          not_solid    candidates A does not hold, dropped because R holds them fewer than thre_solid times (0 when solid is NULL)
 *          selected     candidates - in_absent - not_solid = the keys of dst
 * S is swept in pieces of at most 2^24 slots (JASPER_SELECT_PIECE=<slots>, 1 .. 2^24, overrides it: a test hook); a piece's keys reach
 * dst through the import that jasper_table_import_device is, so dst grows as any table does, and JASPER_ERR_CAPACITY is that import's.
 * device_seconds (may be NULL): device time of the select sweeps, HIP events; the imports are not in it. */
int jasper_table_select(jasper_table *dst, jasper_table *src, jasper_table *absent, jasper_table *solid /* may be NULL */, uint32_t thre_src, uint32_t thre_solid,
                        uint64_t out4[4] /* candidates, in_absent, not_solid, selected */, double *device_seconds);

/* The counting sibling of the select: dst = src - minus as a table.  src (S), minus (M) and dst are whole tables of the same k on the same
 * device, all handles different, narrow or wide, of any sizes; dst holds no key.  Anything else is JASPER_ERR with a message that names
 * the cause, before any table is touched.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  Counting is additive: where M counts a part of the
 * sequences S counts, dst counts the rest, key by key and exactly (jasper_count_binned: all reads - the other bin = own bin + unknown).
 *
 * For every distinct key x of S, with the full 64-bit counts S[x] and M[x] (0 for a key M lacks -- not the 32-bit clamp of the lookups):
 * dst[x] = S[x] - M[x] where that is above 0, otherwise x is not in dst.  S and M are not modified.
 *   out5 = swept      the keys of S
 *          matched    those M holds
 *          dropped    those with M[x] == S[x]
 *          underflow  those with M[x] > S[x]: left out of dst
 *          kept       swept - dropped - underflow = the keys of dst
 * dst's occurrences (jasper_table_info) are the sum of its counts: the k-mer occurrences of the sequences S counts and M does not.
 * M is a sub-multiset of S iff underflow == 0 and matched == the distinct keys of M; the call returns the table either way.
 * S is swept in pieces of at most 2^24 slots (JASPER_SUBTRACT_PIECE=<slots>, 1 .. 2^24, overrides it: a test hook); a piece's keys reach
 * dst through the select's import.  device_seconds (may be NULL): device time of the subtract sweeps, HIP events; the imports are not in it. */
int jasper_table_subtract(jasper_table *dst, jasper_table *src, jasper_table *minus, uint64_t out5[5] /* swept, matched, dropped, underflow, kept */,
                          double *device_seconds);

/* Trio read binning: per READ of the child, how many of its windows hold a k-mer that only the mother's reads have and how many hold one
 * that only the father's have -- what TrioCanu-style binning sorts the child's reads by.  The tables are the scan's mat (M) and pat (P)
 * above: whole tables of the same k on the same device, different handles; thre_mat and thre_pat are each at least 1.  No table is
 * modified.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  It is the hap-mer scan without a child table, laid
 * out for reads: jasper_hapmer_scan of the same reads gives the same two numbers (counters 2 and 3 of a sequence), but its work is cut per
 * sequence, in tiles a read of 150 bases fills to 3 %, and it takes a pointer per read.  Here the text is FLAT and the work is cut over it.
 *
 * Input.  n_reads reads packed back to back, no separator bytes: read i = text[offsets[i] .. offsets[i+1]); offsets is a host array of
 * n_reads+1 entries, non-decreasing, offsets[0] >= 0 (bytes before offsets[0] and from offsets[n_reads] on are not read).  For the tables' k:
 *   window                 k consecutive bytes of ONE read: read i has max(0, len_i - k + 1) of them.  No window spans two reads
 *   valid                  iff all its k bytes are ACGTacgt (case folded)
 *   m, p                   the counts of its canonical k-mer in M and P, each clamped to 2^32-1
 *   out_mat[i]             the valid windows of read i with m >= thre_mat and p == 0
 *   out_pat[i]             the valid windows of read i with p >= thre_pat and m == 0
 * Reads shorter than k (empty ones too, several in a row too) are legal and give zeros; n_reads == 0 is legal and writes nothing.  The
 * result is the same on every call.  out_mat and out_pat are host arrays of n_reads words.  device_seconds (may be NULL): device time of
 * the start-bit pass and the scan kernel, HIP events.  The kernels run on the mother's stream.
 *   jasper_read_bins         the text in host memory (text[offsets[0] .. offsets[n_reads]) is uploaded)
 *   jasper_read_bins_device  the text in HBM on the tables' device, at any alignment; offsets still a host array
 * Limits (the index arithmetic's): at most 2^31-1 reads and 2^43 text bytes per call, at most 2^32-1 windows per read.
 * JASPER_ERR with a message that names the cause: a different k, different devices, the same handle twice, an attached (owner-sharded)
 * table, a threshold of 0, offsets that decrease or start below 0, a NULL text with offsets[n_reads] > offsets[0], input beyond the limits. */
int jasper_read_bins(jasper_table *mat, jasper_table *pat, int64_t n_reads, const char *text, const int64_t *offsets, uint32_t thre_mat, uint32_t thre_pat,
                     uint32_t *out_mat, uint32_t *out_pat, double *device_seconds);
int jasper_read_bins_device(jasper_table *mat, jasper_table *pat, int64_t n_reads, const void *d_text, const int64_t *offsets /* host */, uint32_t thre_mat,
                            uint32_t thre_pat, uint32_t *out_mat, uint32_t *out_pat, double *device_seconds);

/* The same from the child's read FILES: a chunk of raw FASTQ / FASTA text is uploaded as it stands, kernels find its lines, verify the
 * record shape, pack the sequences back to back and write the offsets, and the binning above runs on what they packed.  Only the small
 * per-record arrays come back.  An EXTENSION like the binning; beside the read feed (jasper_read_feed_*), which marks a record's end in
 * the base stream and hands out no offsets.  What it computes is what the host parser of jasper_amd/triobin.py computes for the same
 * (text, eof):
 *   line       ends at a line feed; with eof a last line without one counts.  A CR directly before a line's end (the line feed, or the
 *              text's end with eof) is not part of the line; a CR anywhere else is a byte like any other
 *   FASTQ      format 0.  A record is four lines, counted from the text's first byte, which the caller guarantees begins a record: line 4i
 *              begins with @, line 4i+2 with +, lines 4i+1 and 4i+3 have equal lengths (a quality line may begin with @ or +).  Without
 *              eof a trailing partial record is not used; with eof a line count that is no multiple of 4 is malformed
 *   FASTA      format 1.  A line is a header iff it begins with >; a record is a header and every line up to the next header, its sequence
 *              those lines' bytes without line ends (blank lines give nothing, a header alone is an empty read).  Without eof the last
 *              record of the text is not used: its end is not known
 *   used       the bytes whole records cover; n_records how many.  The caller passes text + used on with the next chunk
 *   status     0 clean, 1 malformed with bad_record = the first record that fails a check, or n_records when the file ends inside a
 *              record.  Malformed is no error (JASPER_OK); nothing is binned then and nothing can be fetched
 *   device_seconds (may be NULL) two numbers, HIP events: [0] the index and pack kernels, [1] the start-bit pass and the scan kernel
 * The results stay in mat's workspace until its next binning call of any kind.  jasper_read_text_fetch copies them out: rec_start[n_records
 * + 1] (record i = text[rec_start[i] .. rec_start[i+1]), the last entry = used), head_end[n_records] (where the header line ends, before
 * a CR), lens[n_records], out_mat / out_pat as jasper_read_bins gives them for the packed sequences, and, where out_seq is not NULL, those
 * sequences (sum of lens bytes; for tests).  n_records must be what the call before returned: anything else is JASPER_ERR.
 * Limits: n < 2^31 text bytes per call (more is JASPER_ERR before the text is looked at).  JASPER_ERR also for what jasper_read_bins
 * refuses of the tables and thresholds, a format other than 0 / 1, a NULL text with n > 0. */
int jasper_read_text_bins(jasper_table *mat, jasper_table *pat, const char *text /* host */, int64_t n, int eof, int format, uint32_t thre_mat, uint32_t thre_pat,
                          int64_t *used, int64_t *n_records, int *status, int64_t *bad_record, double *device_seconds /* [2] */);
int jasper_read_text_fetch(jasper_table *mat, int64_t n_records, int64_t *rec_start, int64_t *head_end, int64_t *lens, uint32_t *out_mat, uint32_t *out_pat,
                           uint8_t *out_seq /* may be NULL */);

/* The reads of chosen BINS of a packed batch counted into tables of their own, while the batch is in HBM.  An EXTENSION like the binning:
 * that says which bin a read belongs to, this makes the k-mer table of "the reads of bins {..}".
 *
 * Input.  n_reads reads packed back to back as jasper_read_bins takes them (offsets: a host array of n_reads+1 entries), and codes, a host
 * array of one bin code 0 .. 2 per read.  n_sinks (1 .. 3) SINKS: sink s is the table sinks[s] and masks[s], a value 1 .. 7 with bit b
 * set iff the sink takes the reads of code b.  The sinks are whole tables of one k on one device, all handles different.
 * Output.  Every sink's table has been added the canonical k-mers of the reads whose code is in its mask, exactly as
 * jasper_count_bases_device counts a stream of those reads, in input order, each followed by one non-base byte: no k-mer spans two reads,
 * a read shorter than k (empty ones too) gives none.  The stream is gathered on the GPU in pieces of whole reads of at most 2^28 bytes
 * (JASPER_BINCOUNT_PIECE=<bytes> overrides it: a test hook); a longer read is a piece of its own.  A sink's kernels run on its stream.
 *   out           3 numbers per sink: the reads, the bases and the k-mer occurrences gathered into it
 *   seconds       (may be NULL) 2 numbers per sink: device time of the gather kernel alone (HIP events), wall time of the counting calls
 *   jasper_count_binned         the text in host memory (text[offsets[0] .. offsets[n_reads]) is uploaded)
 *   jasper_count_binned_device  the text in HBM on the sinks' device, at any alignment, complete when the call is made
 *   jasper_read_text_count      the packed sequences and offsets that the last jasper_read_text_bins / jasper_gz_text_bins call left in
 *                               mat's workspace: no sequence visits the host.  n_records must be what that call returned; pat (may be
 *                               NULL) is that call's other table, and neither may be a sink
 * n_reads == 0 is legal and counts nothing.  JASPER_ERR with a message that names the cause: a sink of another k or on another device,
 * an attached (owner-sharded) sink, one table in two sinks, a sink that is mat or pat, a code above 2, a mask of 0 or above 7, offsets
 * that decrease or start below 0, an n_records that is not the binning call's, input beyond jasper_read_bins' limits.
 * JASPER_ERR_CAPACITY is the counting call's. */
int jasper_count_binned(int n_sinks, jasper_table *const *sinks, const uint32_t *masks, int64_t n_reads, const char *text /* host */, const int64_t *offsets,
                        const uint8_t *codes, uint64_t *out /* [3 * n_sinks] */, double *seconds /* [2 * n_sinks] */);
int jasper_count_binned_device(int n_sinks, jasper_table *const *sinks, const uint32_t *masks, int64_t n_reads, const void *d_text, const int64_t *offsets /* host */,
                               const uint8_t *codes, uint64_t *out, double *seconds);
int jasper_read_text_count(jasper_table *mat, jasper_table *pat /* may be NULL */, int64_t n_records, const uint8_t *codes, int n_sinks, jasper_table *const *sinks,
                           const uint32_t *masks, uint64_t *out, double *seconds);

/* A gzip text session: ONE .gz read file inflated on the GPU (the device inflater of the counting path) whose text goes to the read-text
 * path inside HBM.  The session belongs to `mat`: its device and stream, its workspace; no counting call may run on `mat` while a session
 * is open, and a session is closed before its table.  The environment hooks of the device inflater (JASPER_INGEST_GZ_DEVICE_CHUNK,
 * _SLAB_MB, _FALSE_STARTS) hold.  open is JASPER_ERR with a message when the file is not for the device inflater -- not a regular file, no
 * valid gzip header, no device memory -- and the caller reads it the ordinary way.
 * bins: one chunk.  Its text is the unused tail of the call before (n - used bytes, kept in a buffer of the session's) and up to `want`
 * more inflated bytes; then everything is what the read-text call does with that text, eof = 1 when the inflater has ended, and the
 * results are fetched with the read-text fetch.
 *   format     in / out: 0 = decide from the text's first byte ('@' FASTQ, '>' FASTA), 1 = FASTQ, 2 = FASTA.  A first byte that is neither
 *              gives status 2 (no format): nothing is parsed, format stays 0
 *   status     0 clean, 1 malformed (as the read-text call has it; the text stays whole for the next call), 2 no format
 *   device_seconds (may be NULL) three numbers, HIP events: [0], [1] as the read-text call has them, [2] this call's pull of inflated
 *              text: events around it, so the inflater's kernels and copies and the host's stitching and waits between them
 * Limits: the tail and want together stay below 2^31 bytes (more is JASPER_ERR before anything is inflated).  An inflater error (CRC or
 * length, truncated or damaged data) is JASPER_ERR with a message that names the file, and every later call of the session fails too.
 * copy: bytes [from, from + len) of the current bins call's text to host memory (a malformed chunk for the host parser; header lines).
 * The text lies in mat's workspace: copy before any other read-text call on mat.  A session serves bins calls or route calls (below),
 * not both: the other kind is JASPER_ERR.
 * stats: the six numbers the last-inflate call reports, for this session. */
typedef struct jasper_gz_text jasper_gz_text;
int jasper_gz_text_open(jasper_table *mat, const char *path, jasper_gz_text **out);
void jasper_gz_text_close(jasper_gz_text *h);
int jasper_gz_text_bins(jasper_gz_text *h, jasper_table *mat, jasper_table *pat, int64_t want, int *format, uint32_t thre_mat, uint32_t thre_pat, int64_t *n, int *eof,
                        int64_t *used, int64_t *n_records, int *status, int64_t *bad_record, double *device_seconds /* [3] */);
int jasper_gz_text_copy(jasper_gz_text *h, int64_t from, int64_t len, uint8_t *dst /* host */);
int jasper_gz_text_stats(jasper_gz_text *h, uint64_t stats[6]);

/* Routing: a text of n bytes is cut into n_seg segments by bounds[n_seg + 1] (bounds[0] = 0, bounds[n_seg] = n, no value below the one
 * before it; a segment may be empty), segment i has bin code bins[i] in 0..2.  out0 / out1 / out2 (host, room for n bytes each) get the
 * segments of bin 0 / 1 / 2 back to back in input order, out_bytes[3] their byte totals: every text byte leaves exactly once.
 * mismatches = the segments i >= check_from (0 or 1) that hold a byte and whose first byte is not `first`; the bytes are routed all the
 * same.  device_seconds (may be NULL): the kernels' time, HIP events.  JASPER_ERR for bounds or bin codes that are not as above, n or
 * n_seg of 2^31 or more, before any kernel runs.
 * The session's route pulls the next `want` inflated bytes into HBM instead of taking a host text, and returns how many came in `got`;
 * when got != bounds[n_seg] nothing is routed (JASPER_OK: the file is not the one the bounds were made for).  `t` is the session's table.
 * device_seconds there: two numbers, [0] the kernels, [1] this call's pull, as the bins call times it. */
int jasper_route_text(jasper_table *t, const uint8_t *text /* host */, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from,
                      uint8_t *out0, uint8_t *out1, uint8_t *out2, int64_t out_bytes[3], int64_t *mismatches, double *device_seconds);
int jasper_gz_text_route(jasper_gz_text *h, jasper_table *t, int64_t want, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from,
                         uint8_t *out0, uint8_t *out1, uint8_t *out2, int64_t out_bytes[3], int64_t *got, int64_t *mismatches, double *device_seconds /* [2] */);

/* Compression: a text of n bytes (host) as BGZF members (SAM specification 4.1), made on the GPU.  The text is cut into blocks of 65280
 * bytes, the last may be short; every block becomes one complete gzip member -- the 18-byte header 1f 8b 08 04 00000000 00 ff 06 00 42 43
 * 02 00 <member bytes - 1 as u16>, one final deflate block, CRC-32 and ISIZE of the block's text -- of at most 65536 bytes, and the members
 * lie back to back in `out` (host, room for out_cap bytes), *out_bytes of them.  n = 0 gives no member: the 28-byte empty member that ends a
 * BGZF file is the file writer's, once per file.  Per block the cheapest in bytes of three encodings is written: a greedy LZ77 parse
 * (matches of 3..258 bytes at distances up to 32768, found through a hash of three bytes and the byte before) under dynamic Huffman codes,
 * the literals alone under a dynamic Huffman code, or a stored block; so a member never exceeds its text by more than 31 bytes and
 * jasper_deflate_bound(n) = n + 31 * blocks always suffices for out_cap (-1 for n < 0).  Members that do not fit out_cap are JASPER_ERR,
 * as is n of 2^31 or more.  The same text gives the same bytes in every call.
 *   counters[6] (may be NULL): blocks, stored blocks, literal-only blocks, LZ blocks, and the LZ blocks' matches and matched bytes
 *   device_seconds (may be NULL): the kernels' time, HIP events
 * The two routing calls with the suffix _gz take what jasper_route_text / jasper_gz_text_route take and route as they do, but out0 / out1 /
 * out2 (room for out_cap[b] bytes; jasper_deflate_bound(n) always suffices) get the BGZF members of each bin's bytes: the routed bytes stay
 * in HBM, the compressor runs on the three ranges, only the members are copied down.  out_bytes[3] = the members' bytes, raw_bytes[3] = the
 * routed bytes (what out_bytes is in the plain calls); a bin without a byte gets no member.  counters[6]: the three bins' sums.
 * device_seconds: [0] the route kernels, [1] the compressor's kernels; from a session [0] the route kernels, [1] the pull, [2] the compressor. */
int64_t jasper_deflate_bound(int64_t n);
int jasper_deflate_bgzf(jasper_table *t, const uint8_t *text /* host */, int64_t n, uint8_t *out /* host */, int64_t out_cap, int64_t *out_bytes, uint64_t counters[6],
                        double *device_seconds);
int jasper_route_text_gz(jasper_table *t, const uint8_t *text /* host */, int64_t n, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from,
                         uint8_t *out0, uint8_t *out1, uint8_t *out2, const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *mismatches,
                         uint64_t counters[6], double *device_seconds /* [2] */);
int jasper_gz_text_route_gz(jasper_gz_text *h, jasper_table *t, int64_t want, int64_t n_seg, const int64_t *bounds, const uint8_t *bins, int first, int check_from,
                            uint8_t *out0, uint8_t *out1, uint8_t *out2, const int64_t out_cap[3], int64_t out_bytes[3], int64_t raw_bytes[3], int64_t *got,
                            int64_t *mismatches, uint64_t counters[6], double *device_seconds /* [3] */);

/* Variant scan: WHERE on the sequences the reads hold a solid single-base alternative to the base the sequence has -- the second allele
 * of a diploid genome that a one-haplotype assembly cannot show, or a substitution the polisher has not made.  One resident table (whole,
 * wide, or attached owner-sharded) and a set of sequences, scanned densely on the GPU as jasper_kmer_report scans them.
 *
 * What it replaces: nothing -- this is an EXTENSION.  The reference meets the situation inside its walk (src/jasper.py: fixdiploid,
 * fix_k_case_sub), acts on it there and reports nothing.  For a sequence s of n bytes (case folded), the table's k and thre >= 1
 * (thre == 0 is JASPER_ERR):
 *   position p  evaluated  iff k-1 <= p <= n-k and all 2k-1 bytes s[p-k+1 .. p+k-1] are ACGTacgt: the k windows that cover p all exist and
 *                          are valid
 *   m(p, x)                for a base x: the minimum over those k windows of the table's count of the window's canonical k-mer with byte p
 *                          replaced by x, counts clamped to 2^32-1 as jasper_lookup clamps them
 *   ref, ref_min           the folded s[p], m(p, ref)
 *   record                 for every x != ref with m(p, x) >= thre one {seq, pos = p, ref, alt = x, ref_min, alt_min = m(p, x), kind}:
 *                          kind het (1) when ref_min >= thre -- both alleles are solid; kind error (2) when ref_min < thre -- only the
 *                          alternative is solid, a substitution that has not been made
 *   per sequence           three counters: evaluated positions, het records, error records
 * Records are ordered by (seq, pos, alt in A < C < G < T order); the key is unique, so the list is identical on every call.  Sequences
 * shorter than 2k-1 (empty ones too) are legal and give zeros.  The table is not modified.
 *
 * Limits: only ISOLATED substitutions are reported.  Two differences less than k apart hide each other, because every window that covers
 * one of them holds the other allele of the other (jasper_compound_scan lists such clusters where the sequence is wrong,
 * jasper_indel_scan_clusters where both alleles are solid).  Insertions and deletions are not reported here: jasper_indel_scan below lists
 * them (same-base insertions and any deletion of up to 16 bytes) from the same dense scan, together with everything this call returns.
 *
 * On the device a dense scan probes, per window, the window's last base replaced by each of the other three; a solid one makes the
 * window's end a candidate (a necessary condition: one of the k terms of m), and a second kernel checks each candidate's k windows.  The
 * library sizes the candidate list by itself and repeats the scan once when there were more (jasper_varscan_retried).
 *   jasper_variant_scan         sequences in host memory
 *   jasper_variant_scan_device  sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the table's device; offsets is a host array of
 *                               n_seqs+1 entries
 *   jasper_varscan_counts       out3 = evaluated, het, error of one sequence
 *   jasper_varscan_records      the record list (owned by the result); ref / alt are the letters 'A', 'C', 'G', 'T'
 *   jasper_varscan_candidates   what the dense scan handed to the check (>= records)
 *   jasper_varscan_seconds      device time of the scan's kernels (HIP events) */
typedef struct jasper_varscan jasper_varscan;
typedef struct jasper_variant { int64_t pos; uint32_t seq, ref_min, alt_min; uint8_t ref, alt, kind, pad; } jasper_variant; /* 24 B; ref/alt = 'A','C','G','T' */
int jasper_variant_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, jasper_varscan **out);
int jasper_variant_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, jasper_varscan **out);
int jasper_varscan_num_seqs(const jasper_varscan *r);
int jasper_varscan_counts(const jasper_varscan *r, int seq, uint64_t out3[3]);   /* evaluated, het, error */
int jasper_varscan_records(const jasper_varscan *r, const jasper_variant **recs, uint64_t *n);
int jasper_varscan_candidates(const jasper_varscan *r, uint64_t *n);             /* what the dense scan handed to the check */
double jasper_varscan_seconds(const jasper_varscan *r);                          /* device time, HIP events */
int jasper_varscan_retried(const jasper_varscan *r);
void jasper_varscan_free(jasper_varscan *r);

/* Indel scan: WHERE on the sequences the reads hold a solid insertion or deletion against the sequence -- a length difference between the
 * haplotypes of a diploid genome, or a length error the polisher has not repaired.  The length-changing half of the variant scan: the
 * same table (whole, wide, or attached owner-sharded), the same dense scan, and a result that also holds what jasper_variant_scan returns.
 *
 * What it replaces: nothing -- this is an EXTENSION.  The reference repairs such differences inside its walk (src/jasper.py: fix_insert,
 * fix_del, fix_same_base_del, fix_same_base_insertion) and reports nothing.  For a sequence s of n bytes (case folded), the table's
 * k >= 2, thre >= 1 and max_len in 1..16 (anything else is JASPER_ERR with a message that names the argument, even with nothing to scan);
 * F = s[p-k+1 .. p-1], the k-1 bytes before p; cnt() = the table's count of a canonical k-mer, clamped to 2^32-1 as jasper_lookup clamps:
 *   ins(p, x, L)   for 1 <= L <= max_len and a base x != s[p]: the reads hold x repeated L times between bytes p-1 and p.
 *                  evaluated  iff k-1 <= p <= n-k+1 and all bytes s[p-k+1 .. p+k-2] are ACGTacgt
 *                  alt_min    the minimum of cnt over the k+L-1 windows of  A = F + x^L + s[p .. p+k-2]
 *                  ref_min    the minimum of cnt over the k-1 windows of s that start at p-k+1 .. p-1 (those that hold s[p-1] and s[p])
 *                  Only same-base insertions are in scope (what fix_same_base_del repairs); because x != s[p] each has exactly one
 *                  representation, the right-most one.
 *   del(p, L)      for 1 <= L <= max_len and s[p+L] != s[p]; x = s[p+L]: the reads lack s[p .. p+L-1] (any deleted string).
 *                  evaluated  iff k-1 <= p, p+L+k-2 <= n-1 and all bytes s[p-k+1 .. p+L+k-2] are bases
 *                  alt_min    the minimum of cnt over the k-1 windows of  A = F + s[p+L .. p+L+k-2]
 *                  ref_min    the minimum of cnt over the k+L-1 windows of s that start at p-k+1 .. p+L-1 (those that hold a deleted byte)
 *                  s[p+L] != s[p] is right-normalisation again.
 *   record         a hypothesis that is evaluated and has alt_min >= thre gives one {seq, pos = p, type, len = L, base = x, ref_min,
 *                  alt_min, kind}: kind het (1) when ref_min >= thre, error (2) otherwise, as for substitutions.  Hypotheses are
 *                  independent: a substitution, an insertion and several deletions at one p can all be records (low-complexity sequence).
 *   per sequence   four counters: ins_het, ins_error, del_het, del_error
 * Records are ordered by (seq, pos, type, len, base); the key is unique, so the list is identical on every call.  Sequences shorter than
 * 2k-2 (empty ones too) are legal and give zeros.  The table is not modified.
 *
 * Limits: insertions of mixed bases are reported only by jasper_indel_scan_mixed below, lengths above 16 are not reported, and, as for
 * substitutions, two differences less than k apart hide each other (the error side of such clusters: jasper_compound_scan; the het
 * side: jasper_indel_scan_clusters below).
 *
 * On the device the variant scan's dense scan runs unchanged: its candidate (p, x) -- the window that ends at p is solid with its last
 * base replaced by x -- is the first k-mer of A for ins(p, x, L) and for del(p, L) with s[p+L] == x.  One more kernel tests these
 * hypotheses per candidate, then the substitution check runs over the same candidates.  The record list can hold more records than there
 * are candidates; the library sizes it by itself and repeats the indel check (not the scan) once when there were more
 * (jasper_indelscan_retried).
 *   jasper_indel_scan              sequences in host memory
 *   jasper_indel_scan_device       sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the table's device; offsets is a host array of
 *                                  n_seqs+1 entries
 *   jasper_indelscan_counts        out4 = ins_het, ins_error, del_het, del_error of one sequence
 *   jasper_indelscan_records       the record list (owned by the result)
 *   jasper_indelscan_variants      the substitution result, owned by the indel result (do not free it): counts, records and candidates
 *                                  equal those of jasper_variant_scan on the same input
 *   jasper_indelscan_seconds       device time of the scan and all check kernels (HIP events)
 *   jasper_indelscan_check_seconds ... of the indel check alone
 *   jasper_indelscan_lookups       table lookups the indel check made (for measurements: time per lookup) */
typedef struct jasper_indelscan jasper_indelscan;
typedef struct jasper_indel {
    int64_t pos;
    uint32_t seq, ref_min, alt_min;
    uint16_t len;
    uint8_t type /* 1 ins, 2 del */, base /* 'A','C','G','T': x */, kind /* 1 het, 2 error */, pad[7] /* 0 */;
} jasper_indel; /* 32 B */
int jasper_indel_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_indelscan **out);
int jasper_indel_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_indelscan **out);
int jasper_indelscan_num_seqs(const jasper_indelscan *r);
int jasper_indelscan_counts(const jasper_indelscan *r, int seq, uint64_t out4[4]);   /* ins_het, ins_error, del_het, del_error */
int jasper_indelscan_records(const jasper_indelscan *r, const jasper_indel **recs, uint64_t *n);
const jasper_varscan *jasper_indelscan_variants(const jasper_indelscan *r);
double jasper_indelscan_seconds(const jasper_indelscan *r);                         /* device time, HIP events */
double jasper_indelscan_check_seconds(const jasper_indelscan *r);
int jasper_indelscan_lookups(const jasper_indelscan *r, uint64_t *n);
int jasper_indelscan_retried(const jasper_indelscan *r);
void jasper_indelscan_free(jasper_indelscan *r);

/* Mixed-base insertions: jasper_indel_scan plus the insertions of ANY string of up to max_len bases.
 *
 * What it replaces: nothing -- an EXTENSION of the extension above.  jasper_indel_scan lists every deletion but only the insertions of
 * one repeated base, so of a pair of haplotypes that differ by a mixed string it sees the difference from one side only.  The
 * reference's fix_insert / fix_del repair such insertions inside the walk and report nothing.  Notation as above, FRONT =
 * JASPER_INDEL_FRONT = 64:
 *   ins(p, y)      for a string y of L bases, 1 <= L <= max_len <= 16, with y[0] != s[p] (the right-most position: y before p with
 *                  s[p] == y[0] is y[1:] + y[0] before p + 1).
 *                  evaluated  exactly when ins(p, x, L) is: k-1 <= p <= n-k+1 and all bytes s[p-k+1 .. p+k-2] are bases
 *                  alternative string  A = F + y + s[p .. p+k-2], of k+L-1 windows
 *   the search     at a candidate (p, x), evaluated and with cnt(F + x) >= thre:  S_1 = {x};  for t >= 2
 *                      S_t = { yz : y in S_(t-1), z in ACGT, cnt(the last k bytes of F + y + z) >= thre }
 *                  -- the prefixes of length t all of whose windows so far are solid.  It runs t = 1, 2, .. and ends at the first of:
 *                  t > max_len; S_t empty; |S_t| > FRONT.  In the last case the site is COMPLEX: counted once per (p, x), and nothing
 *                  of length >= t is reported there.  Exactly FRONT prefixes are still searched.
 *   record         every y in S_t of a level that was reached, with y != x^t, whose k-1 windows t .. k+t-2 of A are >= thre as well:
 *                  {seq, pos = p, len = t, bases = y, ref_min, alt_min, kind}.  alt_min = the minimum over all k+t-1 windows of A;
 *                  ref_min = the minimum over the k-1 windows of s that start at p-k+1 .. p-1, as for ins(p, x, L); kind het (1) when
 *                  ref_min >= thre, error (2) otherwise.
 *   per sequence   three counters: mixed_het, mixed_error, complex
 * The rule is one of sets, not of a search order: the list, ordered by (seq, pos, len, y), is identical on every call.  Same-base
 * insertions x^t and all deletions stay what jasper_indel_scan reports (complex sites do not touch them); the mixed list never repeats
 * them.  Every accessor above returns for such a result exactly what it returns for jasper_indel_scan on the same input.
 *
 * On the device one more kernel runs between the indel check and the substitution check: one wave per candidate, a breadth-first
 * search with the frontier S_t held one prefix per lane.
 *   jasper_indel_scan_mixed, _mixed_device   as jasper_indel_scan / _device
 *   jasper_indelscan_mixed_counts    out3 = mixed_het, mixed_error, complex of one sequence
 *   jasper_indelscan_mixed_records   the mixed record list (owned by the result)
 *   jasper_indelscan_mixed_seconds   device time of the search kernel (part of jasper_indelscan_seconds)
 *   jasper_indelscan_mixed_lookups   table lookups it made;  jasper_indelscan_mixed_retried: it was repeated with a larger list
 *   jasper_indel_front               JASPER_INDEL_FRONT as the library was built
 * For a result of jasper_indel_scan / _device the mixed accessors give zeros and n = 0. */
#define JASPER_INDEL_FRONT 64
typedef struct jasper_mixed_ins {
    int64_t pos;
    uint32_t seq, ref_min, alt_min, bases /* base i of y in bits 2i..2i+1, A C G T = 0 1 2 3, 0 above 2*len */;
    uint16_t len;
    uint8_t kind /* 1 het, 2 error */, pad[5] /* 0 */;
} jasper_mixed_ins; /* 32 B */
int jasper_indel_scan_mixed(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_indelscan **out);
int jasper_indel_scan_mixed_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_indelscan **out);
int jasper_indelscan_mixed_counts(const jasper_indelscan *r, int seq, uint64_t out3[3]);   /* mixed_het, mixed_error, complex */
int jasper_indelscan_mixed_records(const jasper_indelscan *r, const jasper_mixed_ins **recs, uint64_t *n);
double jasper_indelscan_mixed_seconds(const jasper_indelscan *r);
int jasper_indelscan_mixed_lookups(const jasper_indelscan *r, uint64_t *n);
int jasper_indelscan_mixed_retried(const jasper_indelscan *r);
int jasper_indel_front(void);

/* Het clusters: jasper_indel_scan plus the clusters of heterozygous differences that every single-edit check rejects.
 *
 * What it replaces: nothing -- an EXTENSION of the extension above.  Of two heterozygous differences less than k apart, at p and p2 > p,
 * the dense scan hands over the candidate (p, x), and the substitution and the indel check then reject it: every later window that covers
 * p also covers p2, where the sequence holds the other haplotype's allele.  At p2 there is no candidate at all.  jasper_compound_scan
 * covers only the error side of such clusters, where the sequence's own k-mers are unreliable.  This search starts at the rejected
 * candidates and walks the reads' solid k-mers until they rejoin the sequence -- where, is not known in advance.  Notation: s a sequence
 * of n bytes, case folded; the table's k >= 2, thre >= 1, cluster_len = N in 1..64 (anything else is JASPER_ERR with a message that names
 * the argument, even with nothing to scan); cnt() as above; FRONT = JASPER_INDEL_FRONT = 64:
 *   candidate (p, x)  as the dense scan writes it, unchanged: the window s[p-k+1 .. p] is k bases, x is a base other than s[p], and
 *                  cnt(F + x) >= thre with F = s[p-k+1 .. p-1].
 *   repl(p, R, y)  for 1 <= R <= N and a string y of t bases, 1 <= t <= N, y[0] = x: the reads hold y where the sequence holds
 *                  s[p .. p+R).  The alternative string is A = F + y + G_R with G_R = s[p+R .. p+R+k-2], of k-1+t windows.
 *                  evaluated   all bytes s[p-k+1 .. p+R+k-2] exist and are bases
 *                  ref_min(R)  the minimum of cnt over the k+R-1 windows of s that start at p-k+1 .. p+R-1: those that hold a replaced byte
 *                  R_max(p)    the largest R <= N for which repl is evaluated and ref_min(R) >= thre (both are monotone in R), or 0.  A
 *                              candidate with R_max = 0 is NOT SEARCHED: the sequence's own k-mers there are unreliable, and that site
 *                              is jasper_compound_scan's.
 *                  normal form y[0] != s[p] holds by the candidate; y[t-1] != s[p+R-1], otherwise the same haplotype has a shorter form;
 *                              (R, t) != (1, 1), which is the variant scan's record.  Pure insertions and pure deletions never pass the
 *                              last-base rule and stay the indel scan's: nothing is listed twice.
 *   the search     at a searched candidate: S_1 = {x}.  After level t's record test a prefix y of S_t is CLOSED, and is not extended,
 *                  when the last k-1 bases of F + y equal s[p+R-k+1 .. p+R-1] for some R in 1..R_max: it has been back on the sequence
 *                  for k-1 bases, and whatever differs next is a site of its own with a candidate of its own.
 *                      S_(t+1) = { yz : y in S_t, y not closed, z in ACGT, cnt(the last k bases of F + y + z) >= thre }
 *                  It ends at the first of: t > N; S_t empty; |S_t| > FRONT.  In the last case the candidate is COMPLEX: counted once;
 *                  records of lengths < t stay, nothing of length >= t is listed.
 *   record         every (R, y) with y in a level that was reached, 1 <= R <= R_max and normal form, whose windows t .. t+k-2 of A are
 *                  all >= thre: {seq, pos = p, ref_len = R, len = t, bases = y, ref_min = ref_min(R), alt_min}.  alt_min = the minimum
 *                  over all k-1+t windows of A.  Every record is HET: ref_min >= thre by construction; there is no kind.
 *   per sequence   four counters: searched (candidates with R_max >= 1), sites (searched candidates with at least one record), records,
 *                  complex
 * The rule is one of sets, not of a search order: the list, ordered by (seq, pos, ref_len, len, y), is identical on every call.  Every
 * accessor of jasper_indelscan above returns for such a result exactly what it returns without cluster_len.
 *
 * On the device one more kernel runs over the candidates before the substitution check rewrites them: one wave per candidate, the
 * reference windows first (a candidate with R_max = 0 leaves there), then a breadth-first search with the frontier one prefix per lane
 * and the rejoin tests one R per lane.
 *   jasper_indel_scan_clusters, _clusters_device   as jasper_indel_scan / _device, with mixed (0 or 1: the mixed half as well) and cluster_len
 *   jasper_indelscan_cluster_counts    out4 = searched, sites, records, complex of one sequence
 *   jasper_indelscan_cluster_records   the record list (owned by the result)
 *   jasper_indelscan_cluster_seconds   device time of the search kernel (part of jasper_indelscan_seconds)
 *   jasper_indelscan_cluster_lookups   table lookups it made;  jasper_indelscan_cluster_retried: it was repeated with a larger list
 * For a result of the entry points above the cluster accessors give zeros and n = 0. */
typedef struct jasper_het_cluster {
    int64_t pos;
    uint32_t seq, ref_min, alt_min, ref_len;
    uint64_t bases[2]; /* base i of y in bits 2i..2i+1 of bases[i / 32], A C G T = 0 1 2 3, 0 above 2*len */
    uint16_t len;
    uint8_t pad[6] /* 0 */;
} jasper_het_cluster; /* 48 B, laid out like jasper_compound */
int jasper_indel_scan_clusters(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int mixed, int cluster_len,
                               jasper_indelscan **out);
int jasper_indel_scan_clusters_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, int mixed,
                                      int cluster_len, jasper_indelscan **out);
int jasper_indelscan_cluster_counts(const jasper_indelscan *r, int seq, uint64_t out4[4]);   /* searched, sites, records, complex */
int jasper_indelscan_cluster_records(const jasper_indelscan *r, const jasper_het_cluster **recs, uint64_t *n);
double jasper_indelscan_cluster_seconds(const jasper_indelscan *r);
int jasper_indelscan_cluster_lookups(const jasper_indelscan *r, uint64_t *n);
int jasper_indelscan_cluster_retried(const jasper_indelscan *r);

/* Compound scan: WHAT the reads hold in place of a cluster of differences that hide each other from the two scans above.
 *
 * What it replaces: nothing -- an EXTENSION.  Two differences less than k apart leave no solid single-edit alternative: every window that
 * covers one of them holds the sequence's wrong base at the other, so jasper_variant_scan and jasper_indel_scan stay silent, and all that
 * shows is a run of unreliable windows in jasper_kmer_report.  The reference repairs such clusters inside its walk where it can and
 * reports nothing.  The read table is a de Bruijn graph of the reads; this scan walks its solid k-mers from the left flank of such a run
 * and lists every string that rejoins the sequence on the right flank: several substitutions, or a substitution and a length error.
 * For a sequence s (case folded), the table's k >= 2, thre >= 1 and max_len in 1..64 (anything else is JASPER_ERR with a message that
 * names the argument, even with nothing to scan); cnt() = the table's count of a canonical k-mer, clamped to 2^32-1 as jasper_lookup
 * clamps; FRONT = JASPER_COMPOUND_FRONT = JASPER_INDEL_FRONT = 64:
 *   sites          a maximal run of unreliable windows exactly as jasper_kmer_report lists it, (start, n_kmers, min_count); R =
 *                  n_kmers - k + 1.  The run is a SITE when 1 <= R <= max_len and LONG when R > max_len: long runs are counted and not
 *                  searched.  Runs with n_kmers < k are neither: pure insertions, or runs that end at an edge or a non-base byte; they
 *                  stay with the other scans.  For a site a = start + k - 1, q = start + n_kmers, F = s[a-k+1 .. a-1] and G =
 *                  s[q .. q+k-2]: both lie inside the bytes the run's windows cover, so they are bases and in bounds, at a sequence's
 *                  first and last window too.  The sequence's own R bytes s[a .. q) are what is replaced.
 *   repl(a, R, y)  the reads hold the string y in place of those R bytes; its alternative string is A = F + y + G, of k-1+|y| windows.
 *   the search     S_0 = {empty};  S_t = { yz : y in S_(t-1), z in ACGT, cnt(the last k bases of F + y + z) >= thre }.  It runs t = 1,
 *                  2, .. and ends at the first of: t > max_len; S_t empty; |S_t| > FRONT.  In the last case the site is COMPLEX: counted
 *                  once; records of lengths < t that were found stay, nothing of length >= t is listed.
 *   record         every y in an S_t that was reached whose windows t .. t+k-2 of A -- those that hold a base of G -- are >= thre as
 *                  well: {seq, pos = a, ref_len = R, len = t, bases = y, ref_min, alt_min}.  alt_min = the minimum of cnt over all
 *                  k-1+t windows of A; ref_min = the run's min_count, below thre by construction: every record is an ERROR, there is no
 *                  kind.  Exception: R = 1 and t = 1 is the variant scan's error and is never listed.  Deletions (t = 0) are not
 *                  searched: they stay the indel scan's.  Window 0 of A is F + y[0] and the sequence's own window there is unreliable,
 *                  so y[0] != s[a] needs no rule of its own; the same holds for y's last base and s[q-1].
 *   per sequence   five counters: sites, bridged (sites with at least one record), records, long, complex
 * The rule is one of sets, not of a search order: the list, ordered by (seq, pos, len, y), is identical on every call.  The table is
 * not modified.
 *
 * Limits: compound HET sites -- where both alleles are solid there is no unreliable run -- are not listed here but by
 * jasper_indel_scan_clusters above; replacements longer than 64 bases are not listed.
 *
 * On the device jasper_kmer_report's scan runs unchanged; the host picks the sites and the long runs from its runs, and one more
 * kernel searches the sites, one wave each, with the frontier S_t held one prefix per lane.  With no site nothing more is allocated
 * or launched.  The result holds the whole report, so one call answers both questions.
 *   jasper_compound_scan, _device   as jasper_kmer_report / _device, with max_len
 *   jasper_compscan_counts          out5 = sites, bridged, records, long, complex of one sequence
 *   jasper_compscan_records         the record list (owned by the result)
 *   jasper_compscan_report          the report of the same input, owned by the result (do not free it): every jasper_report_* accessor
 *                                   gives what it gives for jasper_kmer_report
 *   jasper_compscan_seconds         device time (HIP events) of the search kernel alone (*search) and of it and the dense scan (*total)
 *   jasper_compscan_lookups         table lookups the search made;  jasper_compscan_retried: it was repeated with a larger list
 *   jasper_compound_front           JASPER_COMPOUND_FRONT as the library was built */
#define JASPER_COMPOUND_FRONT JASPER_INDEL_FRONT
typedef struct jasper_compscan jasper_compscan;
typedef struct jasper_compound {
    int64_t pos;
    uint32_t seq, ref_min, alt_min, ref_len;
    uint64_t bases[2]; /* base i of y in bits 2i..2i+1 of bases[i / 32], A C G T = 0 1 2 3, 0 above 2*len */
    uint16_t len;
    uint8_t pad[6] /* 0 */;
} jasper_compound; /* 48 B */
int jasper_compound_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, jasper_compscan **out);
int jasper_compound_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, jasper_compscan **out);
int jasper_compscan_num_seqs(const jasper_compscan *r);
int jasper_compscan_counts(const jasper_compscan *r, int seq, uint64_t out5[5]);   /* sites, bridged, records, long, complex */
int jasper_compscan_records(const jasper_compscan *r, const jasper_compound **recs, uint64_t *n);
const jasper_report *jasper_compscan_report(const jasper_compscan *r);
int jasper_compscan_lookups(const jasper_compscan *r, uint64_t *n);
int jasper_compscan_seconds(const jasper_compscan *r, double *search, double *total);
int jasper_compscan_retried(const jasper_compscan *r);
int jasper_compound_front(void);
void jasper_compscan_free(jasper_compscan *r);

/* Repair: the error records of the scans above APPLIED to the sequences on the GPU, in rounds.
 *
 * What it replaces: nothing -- an EXTENSION, and the step after the scans.  An error record is a place where the sequence's own k-mers are
 * unreliable and the reads hold exactly one solid alternative; all of them have one shape, "the reads hold the string y where the sequence
 * holds the R bytes from p on".  The reference repairs inside its walk and never looks again; this call acts on what the walk has left.
 * Given the table's k >= 2, thre >= 1, indel_max_len in 1..16, compound_max_len in 1..64 and rounds = N in 1..8 (anything else is JASPER_ERR
 * with a message that names the argument, even with nothing to scan):
 *   edit           (seq, pos, rlen, y, alt_min, ref_min, source) replaces s[pos .. pos+rlen) by y, 0..64 bases, upper case; q = pos + rlen.
 *                  Only records of kind error become edits (het records are never applied: both alleles are in the reads):
 *                      source 1 sub       variant (p, alt)      pos p, rlen 1, y = alt
 *                      source 2 ins       ins(p, x, L)          pos p, rlen 0, y = x repeated L times
 *                      source 3 del       del(p, L)             pos p, rlen L, y empty
 *                      source 4 mixed     mixed ins(p, y)       pos p, rlen 0, y
 *                      source 5 compound  (a, R, y)             pos a, rlen R, y
 *                  Two records that give the same (seq, pos, rlen, y) are one edit (the lower source stays).
 *   one round      jasper_indel_scan_mixed (it holds the variant scan) and jasper_compound_scan (it holds the report) on the current
 *                  text; their records made edits; then
 *                      ambiguous  edits that share (seq, pos, rlen, |y|, alt_min) and differ in y are all set aside and counted
 *                      order      the rest by (rlen + |y| ascending, alt_min descending, seq, pos, rlen, y)
 *                      accepted   in that order, an edit unless it CONFLICTS with one accepted before it; a conflict is counted and left
 *                                 to the next round's scans.  Two edits a, b of one sequence with (pos_a, q_a) <= (pos_b, q_b) conflict
 *                                 iff pos_b - q_a < k - 1.  A record's evidence is the windows of F + y + G, F and G the sequence's k-1
 *                                 bytes on either side: with at least k-1 bytes between them neither edit lies in the other's flanks, so
 *                                 every window that overlaps an applied y or spans an applied deletion is one a scan has found solid.
 *                  The accepted edits are applied together.  A round that accepts nothing ends the loop.
 *   the loop       at most N rounds.  `before` is the report of round 1's text; `after` the report of the round that accepted nothing,
 *                  or, if round N still applied edits, one more jasper_kmer_report of the final text.
 *   per round      records (edits after duplicates were dropped = accepted + conflicts + ambiguous), accepted, conflicts, ambiguous,
 *                  unreliable_before, unreliable_after: the unreliable windows of all sequences before and after the round's edits.
 *                  unreliable_after = unreliable_before - the unreliable windows w of the old text with pos-k+1 <= w < pos+rlen, summed
 *                  over the accepted edits; that is at least 1 per edit.
 * Bytes that are not replaced stay as they stand: lower case, N, anything.  The table is not modified.
 *
 * Limits: het records are never applied; runs longer than compound_max_len and complex sites stay; ties (ambiguous edits) are skipped.
 *
 * On the device the text is uploaded once and downloaded once: the scans read it in HBM, per round only records come down and edits
 * go up, and one kernel writes the new text into a second buffer -- a gather-copy, one workgroup per tile of jasper_repair_tile_bytes() OUTPUT
 * bytes, 16 bytes per lane, the edits that touch a tile staged through LDS.
 *   jasper_repair, _device          as jasper_kmer_report / _device, with the lengths and rounds; the input text is not written
 *   jasper_apply_edits, _device     the kernel alone on a caller's list: ordered by (seq, pos), every edit inside its sequence, |y| <= 64,
 *                                   no bits above 2|y|, and two edits of one sequence at least one byte apart (pos_b - q_a >= 1); anything
 *                                   else is JASPER_ERR and nothing is launched.  source, round, ref_min and alt_min are not read.
 *   jasper_repair_tile_bytes        output bytes per workgroup of the kernel (tests aim at the seams)
 *   jasper_repaired_num_seqs, _seq  the final sequences (owned by the result)
 *   jasper_repaired_edits           every applied edit, ordered by (round, seq, pos); pos counts in the text that round read (round 1: the
 *                                   input)
 *   jasper_repaired_rounds          one entry per round that scanned (the last accepted nothing, unless the loop ran out of rounds)
 *   jasper_repaired_before, _after  the two reports, owned by the result (do not free them)
 *   jasper_repaired_seconds         device time (HIP events) of the apply kernel alone (*apply) and of it and all scans (*total)
 * For a result of jasper_apply_edits there are no edits, no rounds and two empty reports. */
typedef struct jasper_repaired jasper_repaired;
typedef struct jasper_edit {
    int64_t pos;
    uint32_t seq, ref_min, alt_min, ref_len;
    uint64_t bases[2]; /* base i of y in bits 2i..2i+1 of bases[i / 32], A C G T = 0 1 2 3, 0 above 2*len */
    uint16_t len;
    uint8_t source /* 1 sub, 2 ins, 3 del, 4 mixed, 5 compound */, round /* 1 ..; 0 in a caller's list */, pad[4] /* 0 */;
} jasper_edit; /* 48 B, laid out like jasper_compound */
typedef struct jasper_repair_round { uint64_t records, accepted, conflicts, ambiguous, unreliable_before, unreliable_after; } jasper_repair_round; /* 48 B */
int jasper_repair(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int indel_max_len, int compound_max_len, int rounds,
                  jasper_repaired **out);
int jasper_repair_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int indel_max_len, int compound_max_len, int rounds,
                         jasper_repaired **out);
int jasper_apply_edits(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, const jasper_edit *edits, uint64_t n_edits, jasper_repaired **out);
int jasper_apply_edits_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, const jasper_edit *edits, uint64_t n_edits,
                              jasper_repaired **out);
int jasper_repair_tile_bytes(void);
int jasper_repaired_num_seqs(const jasper_repaired *r);
int jasper_repaired_seq(const jasper_repaired *r, int seq, const char **text, int64_t *len);
int jasper_repaired_edits(const jasper_repaired *r, const jasper_edit **edits, uint64_t *n);
int jasper_repaired_rounds(const jasper_repaired *r, const jasper_repair_round **rounds, uint64_t *n);
const jasper_report *jasper_repaired_before(const jasper_repaired *r);
const jasper_report *jasper_repaired_after(const jasper_repaired *r);
int jasper_repaired_seconds(const jasper_repaired *r, double *apply, double *total);
void jasper_repaired_free(jasper_repaired *r);

/* Duplication map: WHICH other place holds the second copy of every stretch the assembly holds exactly twice.  Two resident tables of the
 * same k on the same device -- `reads` (R, whole or attached owner-sharded) and `assembly` (A, a whole table, a different handle from R,
 * counted from exactly the scanned sequences, as for jasper_copy_report; otherwise JASPER_ERR with a message) -- and a set of sequences,
 * scanned densely on the GPU twice: pass 1 records where A's count-2 k-mers lie, pass 2 joins every window with its mate.
 *
 * What it replaces: nothing -- this is an EXTENSION, the reference has no counterpart.  jasper_copy_report finds the `deficit` runs of a
 * duplicated stretch; this says where the other copy is.  `thre` and `peak` (>= 1, else JASPER_ERR) are jasper_copy_report's.  With
 * offsets[] the starts of the sequences back to back (jasper_dup_map: in the order given, no byte between them):
 *   window i of sequence s    valid     iff all its k bytes are ACGTacgt (case folded)
 *                             strand    1 when the reverse complement is the canonical form (rc < fwd), else 0
 *                             position  offsets[s] + i, encoded with the strand bit as 2 * position + strand
 *   pass 1 (index)            for every valid window whose k-mer has count exactly 2 in A the encoded position goes into the two 64-bit
 *                             side words of the k-mer's slot, with atomicMin and atomicMax: the smallest and the largest encoded position
 *                             seen, whatever the order
 *   pass 2 (join)             c         R's count of the window's canonical k-mer, clamped to 2^32-1;  a = A's count
 *                             two-copy  a == 2, the slot's two words are two different positions, and one of them is the window's own;
 *                                       the other is its MATE
 *                             unplaced  a == 2 otherwise: A was not counted from these sequences.  Counted, never paired
 *                             multi     a >= 3.  Counted, never paired: only count exactly 2 is mapped
 *                             orientation  of a two-copy window: `+` when its strand bit equals its mate's, `-` otherwise
 *                             deficit   two-copy, c >= thre and (2 c + peak) div (2 peak) < 2: jasper_copy_report's rule at a = 2
 *   run                       a maximal range of consecutive windows start .. start+n-1 of one sequence that are all two-copy, all of one
 *                             orientation, and whose mates are colinear: mate(start+j) = mate(start) + j for `+`, mate(start) - j for
 *                             `-`.  Two adjacent two-copy windows whose mates are not colinear or whose orientations differ end one run
 *                             and start the next, with no gap between them.  For k >= 2 the mates of a run lie in one sequence
 *   per sequence              seven counters: windows, valid, two_copy, deficit, multi, unplaced, sum_reads (the sum of c over its
 *                             two-copy windows)
 *   jasper_dup_run            start, seq: the run's first window;  n_kmers: its windows;  sum_reads, n_deficit: over them;
 *                             mate_seq, mate_start: the sequence and the LEFTMOST window of the mate stretch (for `-` the mate of the
 *                             run's last window);  strand: 0 for `+`, 1 for `-`;  pad: 0
 * Runs are exact k-mer matches: a substitution in one copy cuts a run into two on one diagonal, k windows apart.  Runs are not chained and
 * nothing is purged.  Sequences shorter than k (empty ones too) are legal and give zeros.  Runs are ordered by (seq, start); every run
 * has its mirror image in the list (start <-> mate_start, seq <-> mate_seq, the same strand and n_kmers).  Neither table is modified and
 * the result is the same on every call.  The library sizes its run buffer by itself and repeats pass 2 once when there were more runs
 * than it had room for (jasper_dupmap_retried).  Tiles are those of the report (jasper_report_tile_windows()).
 *   jasper_dup_map          sequences in host memory
 *   jasper_dup_map_device   sequence i = d_text[offsets[i] .. offsets[i+1]) in HBM on the tables' device; offsets is a host array of
 *                           n_seqs+1 entries
 *   jasper_dupmap_counts    out7 = windows, valid, two_copy, deficit, multi, unplaced, sum_reads of one sequence
 *   jasper_dupmap_runs      the run list (owned by the result)
 *   jasper_dupmap_seconds   device time (HIP events): *index = the side array's fill and pass 1, *scan = pass 2 and the stitching of its
 *                           runs; either pointer may be NULL */
typedef struct jasper_dupmap jasper_dupmap;
typedef struct jasper_dup_run {
    int64_t start; int64_t mate_start; uint64_t n_kmers; uint64_t sum_reads; uint64_t n_deficit; uint32_t seq; uint32_t mate_seq; uint32_t strand; uint32_t pad;
} jasper_dup_run; /* 56 B */
int jasper_dup_map(jasper_table *reads, jasper_table *assembly, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, uint32_t peak,
                   jasper_dupmap **out);
int jasper_dup_map_device(jasper_table *reads, jasper_table *assembly, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, uint32_t peak,
                          jasper_dupmap **out);
int jasper_dupmap_num_seqs(const jasper_dupmap *r);
int jasper_dupmap_counts(const jasper_dupmap *r, int seq, uint64_t out7[7]);   /* windows, valid, two_copy, deficit, multi, unplaced, sum_reads */
int jasper_dupmap_runs(const jasper_dupmap *r, const jasper_dup_run **runs, uint64_t *n);
int jasper_dupmap_seconds(const jasper_dupmap *r, double *index, double *scan);   /* device time, HIP events */
int jasper_dupmap_retried(const jasper_dupmap *r);
void jasper_dupmap_free(jasper_dupmap *r);

/* Gap scan: WHAT the reads hold in place of a scaffold gap, or of a run of unreliable k-mers too long for jasper_compound_scan.
 *
 * What it replaces: nothing -- an EXTENSION (a Sealer-style closure).  A window that holds a non-base byte has no k-mer, so an N run is
 * invisible to every scan above; and jasper_compound_scan counts a run that replaces more than 64 bytes as `long` and stops.  This scan
 * walks the solid k-mers of the reads from the left flank of such a place until they rejoin its right flank, for up to 4096 bases.
 * For a sequence s of n bytes (case folded; a BASE is one of ACGT), the table's k >= 2, thre >= 1, 0 <= max_len <= JASPER_GAP_MAX_LEN =
 * 4096 and max_trim >= 0 (anything else is JASPER_ERR with a message that names the argument, even with nothing to scan); cnt() = the
 * table's count of a canonical k-mer, clamped to 2^32-1 as jasper_lookup clamps; FRONT = JASPER_GAP_FRONT = 64, MAXREC =
 * JASPER_GAP_MAX_RECORDS = 16.  Window w (0 <= w <= n-k) is VALID when its k bytes are bases and SOLID when it is valid and cnt >= thre.
 *   sites          a STRETCH is a maximal run [u0, u1] of windows that are not solid, invalid or unreliable.  Its kind is GAP when it
 *                  holds at least one invalid window, and RUN when it holds none and u1 - u0 + 2 - k > JASPER_GAP_RUN_MIN = 64 -- exactly
 *                  what jasper_compound_scan calls long at its default; the 64 is fixed.  Other stretches are no sites, and RUN sites
 *                  exist only when long_runs is set.  For a site a = u0 + k - 1, q = u1 + 1, F = s[a-k+1 .. a) = the last k - 1 bases of
 *                  the solid window before the stretch, G = s[q .. q+k-1) = the first k - 1 of the solid window after it, and the R =
 *                  q - a bytes s[a .. q) are what a fill replaces.  So N runs with fewer than k bases between them are one site, and
 *                  an unreliable run that touches a gap is part of its site (a dirty contig end).
 *   a site is      EDGE when u0 = 0 or u1 = n-k (no solid window on that side; its trims are 0); else RAGGED when trim_left or
 *                  trim_right exceeds max_trim -- trim_left = (first non-base byte of the stretch) - a, trim_right = q - (last
 *                  non-base byte + 1), both 0 for kind RUN; else SEARCHED.  ref_min = the smallest cnt over the stretch's valid
 *                  windows, 0 when it has none.
 *   the search     per searched site, S_0 = {empty string}.  At level t = 0, 1, 2, .. in this order:
 *                  1 rejoin  every y in S_t whose windows t .. t+k-2 of F + y + G (the k - 1 that hold a base of G) are all solid is a
 *                            record of level t.  If the site's records so far plus this level's exceed MAXREC, the level lists none of
 *                            them, the site is COMPLEX and the search ends (levels = t).
 *                  2 close   every y with t >= k - 1 whose last k - 1 bases equal G leaves S_t: it is a record followed by the whole
 *                            right flank, and what follows it is the sequence.
 *                  3 stop    t = max_len: the search ends, LIMIT if S_t is not empty, else DEAD.  S_t empty: DEAD.  (levels = t)
 *                  4 extend  S_(t+1) = { yz : y in S_t, z in ACGT, cnt(the last k bases of F + yz) >= thre }.  |S_(t+1)| > FRONT: the site
 *                            is COMPLEX, records of lengths <= t stay; S_(t+1) empty: DEAD.  In both cases levels = t + 1, the level
 *                            that could not be formed.
 *   record         {seq, pos = a, ref_len = R, len = t, y, alt_min}; alt_min = the minimum of cnt over all t + k - 1 windows of
 *                  F + y + G.  y is len upper-case letters at bases_off of the result's byte pool.  Ordered by (seq, pos, len, y), and
 *                  the pool holds the strings in that order.
 *   per sequence   nine counters: sites, searched, bridged (at least one record), unique (exactly one record and not complex),
 *                  records, edge, ragged, limit, complex
 * The rule is one of sets, not of a search order: sites, records and bytes are identical on every call.  The table is not modified.
 *
 * Limits: the walk is over EXACT k-mers of the reads (a gap whose true sequence has a read-coverage hole stays open); a het bubble
 * inside a gap multiplies the front, and both alleles are records (such a site is not unique); the closing rule ends a tandem
 * expansion at k - 1 bases -- inside (ACG)x40 at k = 21 the lengths 0, 3, .., 18 are listed and the search ends dead; there are no
 * negative gaps (contig ends that overlap are not joined); at most MAXREC fills of one site are listed.
 *
 * On the device jasper_kmer_report's scan runs unchanged; one more dense kernel lists the runs of invalid windows (no table probe);
 * the host makes the sites; one more kernel searches them, one wave each, and keeps the strings in a per-wave log in global memory
 * (64 bytes a level), not in registers.  With no site to search nothing of the search is allocated or launched.
 *   jasper_gap_scan, _device        as jasper_kmer_report / _device, with max_len, max_trim and long_runs (0 / 1)
 *   jasper_gap_search, _device      the search alone on a caller's sites: a, q, seq and ref_min of each entry are read, the rest is
 *                                   ignored.  They must be in (seq, a) order, no two at one place, with k-1 <= a <= q <= n-(k-1);
 *                                   anything else is JASPER_ERR and launches nothing.  A site whose flanks are not all bases comes back
 *                                   SKIPPED; kind is 0, the trims are 0 and ref_min is the caller's.  The result has no report.
 *   jasper_gapscan_counts           out9 of one sequence, in the order above
 *   jasper_gapscan_sites, _records  the site list, ordered by (seq, a), and the record list (owned by the result)
 *   jasper_gapscan_bases            the byte pool the records' bases_off point into (owned by the result)
 *   jasper_gapscan_report           the report of the same input, owned by the result (do not free it)
 *   jasper_gapscan_seconds          device time (HIP events) of the search kernel (*search), of the invalid-window scan (*runs) and of
 *                                   both and the dense report (*total)
 *   jasper_gapscan_lookups          table lookups the search made;  jasper_gapscan_retried: it was repeated with larger lists
 *   jasper_gap_front, _max_records, _max_len    the constants as the library was built */
#define JASPER_GAP_FRONT 64
#define JASPER_GAP_MAX_RECORDS 16
#define JASPER_GAP_MAX_LEN 4096
#define JASPER_GAP_RUN_MIN 64
enum { JASPER_GAP_KIND_EXPLICIT = 0, JASPER_GAP_KIND_GAP = 1, JASPER_GAP_KIND_RUN = 2 };
enum { JASPER_GAP_DEAD = 1, JASPER_GAP_LIMIT = 2, JASPER_GAP_COMPLEX = 3, JASPER_GAP_EDGE = 4, JASPER_GAP_RAGGED = 5, JASPER_GAP_SKIPPED = 6 };
typedef struct jasper_gapscan jasper_gapscan;
typedef struct jasper_gap_site {
    int64_t a, q;
    uint32_t seq, ref_min, n_records, levels /* the t at which the search ended */, trim_left, trim_right;
    uint8_t kind /* JASPER_GAP_KIND_* */, status /* JASPER_GAP_DEAD .. */, pad[6] /* 0 */;
} jasper_gap_site; /* 48 B */
typedef struct jasper_gap_fill {
    int64_t pos;
    uint64_t bases_off; /* y = len letters from here in jasper_gapscan_bases */
    uint32_t seq, ref_len, len, alt_min;
} jasper_gap_fill; /* 32 B */
int jasper_gap_scan(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, int64_t max_trim, int long_runs,
                    jasper_gapscan **out);
int jasper_gap_scan_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, int64_t max_trim, int long_runs,
                           jasper_gapscan **out);
int jasper_gap_search(jasper_table *t, int n_seqs, const char *const *seqs, const int64_t *lens, uint32_t thre, int max_len, const jasper_gap_site *sites, uint64_t n_sites,
                      jasper_gapscan **out);
int jasper_gap_search_device(jasper_table *t, int n_seqs, const void *d_text, const int64_t *offsets, uint32_t thre, int max_len, const jasper_gap_site *sites,
                             uint64_t n_sites, jasper_gapscan **out);
int jasper_gapscan_num_seqs(const jasper_gapscan *r);
int jasper_gapscan_counts(const jasper_gapscan *r, int seq, uint64_t out9[9]);   /* sites, searched, bridged, unique, records, edge, ragged, limit, complex */
int jasper_gapscan_sites(const jasper_gapscan *r, const jasper_gap_site **sites, uint64_t *n);
int jasper_gapscan_records(const jasper_gapscan *r, const jasper_gap_fill **recs, uint64_t *n);
int jasper_gapscan_bases(const jasper_gapscan *r, const char **bases, uint64_t *n);
const jasper_report *jasper_gapscan_report(const jasper_gapscan *r);
int jasper_gapscan_seconds(const jasper_gapscan *r, double *search, double *runs, double *total);
int jasper_gapscan_lookups(const jasper_gapscan *r, uint64_t *n);
int jasper_gapscan_retried(const jasper_gapscan *r);
int jasper_gap_front(void);
int jasper_gap_max_records(void);
int jasper_gap_max_len(void);
void jasper_gapscan_free(jasper_gapscan *r);

/* The assembly side of src/jasper.sh, natively and by several host threads (no GPU call except jasper_asm_polish):
 *   jasper_asm_open          the assembly FASTA read once into ONE host arena (line ends taken out, contigs back to back).  Returns 1
 *                            (not an error, *out = NULL) for anything but the ordinary file -- '\r', a first byte that is not '>',
 *                            blanks / tabs / non-printable / non-ASCII bytes in sequence lines, odd bytes in header lines, a contig
 *                            name that occurs twice -- for which the caller applies the line-by-line rules of the perl one-liners itself.
 *   jasper_asm_info          *sequence_bytes = `grep -v '^>' $QUERY | tr -d '\n' | wc` third column      src/jasper.sh:132
 *   jasper_asm_contig        name = first whitespace token of the header line WITH its '>' (perl -ane $F[0])  src/jasper.sh:155
 *   jasper_asm_split         perl #1: chunk records ">name:offset" of <= batch_size bases at offsets 0, bs, 2bs ..; perl #2: batch files
 *                            `$prefix.batch.N.fa`, a new one at a record once MORE than batch_size bases are in the current one
 *                            (src/jasper.sh:155-156).  write_files != 0: the files (all, or only_files[0..n_only)) are written by a
 *                            thread of the job while the caller goes on; jasper_asm_split_wait joins it and reports its failure
 *                            ("Splitting files failed", src/jasper.sh:159).
 *   jasper_asm_chunks        per record: contig index, offset, length, batch file (caller's arrays of n_chunks; any may be NULL)
 *   jasper_asm_file_bytes    size of every batch file (what `ls -l` would show; dist.assign_chunks balances by it)
 *   jasper_asm_chunk_text    a record's text: the input (polished = 0) or what jasper_asm_take kept (polished = 1)
 *   jasper_asm_polish        jasper_polish_batch on the records of the listed batch files, read straight from the arena: one
 *                            `jasper.py --query $prefix.batch.N.fa` process per listed file (src/jasper.sh:207-212); result chunk i =
 *                            the i-th record of the files in list order
 *   jasper_asm_pin           optional, any thread (it waits for the GPU runtime to start): registers the arena with the runtime and
 *                            allocates one pinned buffer for the polished text, so that record text crosses PCIe without staging
 *                            copies in either direction
 *   jasper_asm_take          moves the polished text out of the result into the job (for the two writers below); a result of
 *                            jasper_asm_polish leaves its text in HBM until this call copies it
 *   jasper_asm_put           the polished text of one record given by the caller instead (read back from an `_iter*.fixed.fa` of
 *                            an interrupted run; tests)
 *   jasper_asm_write_fixed   `_iter{P-1}_<batch>.fixed.fa`: ">name:offset" + lines of 60            src/jasper.py:120-128,142-147
 *   jasper_asm_polished_lens per record: length of the polished text held (0 if none), and whether it is held
 *   jasper_asm_join          `$QUERY_FN.polished.fasta`: per contig ">name", its records in offset order on ONE line   src/jasper.sh:220
 *                            (contigs in input order; the reference's order is perl's hash order).  all_lens: the polished length of
 *                            EVERY record (NULL: this job holds them all).  mode 1 creates the file at its final size, mode 2 writes
 *                            the records this job holds at their places (several processes, one per GPU, into one file), 3 = both. */
typedef struct jasper_asm jasper_asm;
int jasper_asm_open(const char *path, int threads, jasper_asm **out);
void jasper_asm_close(jasper_asm *a);
int jasper_asm_info(const jasper_asm *a, uint64_t *sequence_bytes, uint64_t *n_contigs, uint64_t *n_bases);
int jasper_asm_contig(const jasper_asm *a, uint64_t i, const char **name, uint64_t *name_len, uint64_t *n_bases);
int jasper_asm_split(jasper_asm *a, uint64_t batch_size, const char *prefix, const uint32_t *only_files, uint32_t n_only, int write_files, int threads,
                     uint64_t *n_chunks, uint64_t *n_files);
int jasper_asm_split_wait(jasper_asm *a);
int jasper_asm_chunks(const jasper_asm *a, uint32_t *contig, uint64_t *ci, uint64_t *len, uint32_t *file);
int jasper_asm_file_bytes(const jasper_asm *a, uint64_t *bytes);
int jasper_asm_chunk_text(const jasper_asm *a, uint64_t chunk, int polished, const char **text, uint64_t *len);
int jasper_asm_polish(jasper_table *t, jasper_asm *a, const uint32_t *files, uint32_t n_files, int solid_thre, int passes, int fix, jasper_result **out);
int jasper_asm_pin(jasper_asm *a, int device);
int jasper_asm_take(jasper_asm *a, jasper_result *r, const uint32_t *files, uint32_t n_files);
int jasper_asm_put(jasper_asm *a, uint64_t chunk, const char *text, uint64_t len);
int jasper_asm_write_fixed(jasper_asm *a, const uint32_t *files, const char *const *out_paths, uint32_t n_files, int threads);
int jasper_asm_polished_lens(const jasper_asm *a, uint64_t *lens, uint8_t *have);
int jasper_asm_join(jasper_asm *a, const char *out_path, const uint64_t *all_lens, int mode, int threads);
/* `$QUERY_FN.fixes.csv` from the per-batch fix CSVs (src/jasper.sh:222-226: awk | awk -F: | sort -k1,1 -k2,2n -k3,3n | awk), byte order
 * for names and for sort's last-resort whole-line comparison.  Returns 1 (not an error, nothing written) when a line holds bytes
 * other than printable ASCII / blank / tab / '\r' or a number of more than 18 digits: the caller applies the rules itself. */
int jasper_merge_fix_csvs(const char *const *paths, uint32_t n_paths, const char *out_path);

/* kernel timing for bench.py: HIP-event time of the last counting call on this table, and its launch count */
int jasper_last_count_timing(jasper_table *t, double *kernel_ms, uint64_t *launches);
/* the same split by kernel stage of the atomic-free counting paths, and which path the last piece took (*path):
 *   1 = one record per occurrence (count_part.hip): part1, part2, region_insert, deferred, (unused x4)
 *   3 = the same with the region lists exchanged between GPUs: part1, part2 by owner (+ dedupe), region_insert, (unused), deferred
 *   0 = count_kernel (global atomics; small pieces)
 * *partitioned_launches of the counted launches took path 1 or 3 (the others ran count_kernel) */
int jasper_last_count_stages(jasper_table *t, double stage_ms[8], uint64_t *partitioned_launches, int *path);

/* A slot array whose IPC handle was given out (jasper_table_ipc_handle) and that the table has outgrown since is kept until
 * this call: the owners make it after they have all attached to the new arrays (jasper_amd/dist.py: shard_tables), so that
 * nothing a peer may still have mapped is ever freed under it.  jasper_table_destroy releases them too. */
int jasper_table_release_retired(jasper_table *t);

/* Host only (no GPU touched): one gzip file inflated by `threads` threads into out_path (or nowhere when out_path is null),
 * the way jasper_count_reads_files reads a large .gz -- the role of `zcat -f` in src/jasper.sh:177.  chunk_bytes = compressed
 * bytes per unit of work (0: default 4 MiB).  *n_out = inflated bytes; *parallel = 1 when the many-thread reader handled the
 * file, 0 when it declined (small file, not a regular gzip file) and zlib's reader was used. */
int jasper_inflate_file(const char *path, int threads, uint64_t chunk_bytes, const char *out_path, uint64_t *n_out, int *parallel);
/* The same on GPU `device` (jasper_amd/csrc/inflate_gpu.hpp): the deflate data is decoded by kernels, the host does the
 * bookkeeping and inflates with zlib only what the device gives back.  Same text and same failures as jasper_inflate_file.
 * chunk_bytes = compressed bytes per decoder (0: default 32 KiB); out_path may be NULL; stats as for jasper_last_inflate. */
int jasper_inflate_file_device(int device, const char *path, uint64_t chunk_bytes, const char *out_path, uint64_t *n_out, uint64_t stats[6]);

#ifdef __cplusplus
}
#endif
#endif
