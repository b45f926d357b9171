"""ctypes binding of libjasper_hip.so (C-ABI declared in include/jasper_hip.h).

There is NO CPU fallback: if the shared library is missing or a call fails, this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (JASPER_AMD_LIB: another build of the same library, for A/B timing of two builds in one run -- tools/ only)
LIB_PATH = os.environ.get("JASPER_AMD_LIB") or os.path.join(_HERE, "libjasper_hip.so")

JASPER_OK = 0
JASPER_ERR = -1
JASPER_ERR_CAPACITY = -2
JASPER_ERR_FORMAT = -3
JASPER_ERR_REFERENCE_EXIT = -4


class FixRec(C.Structure):
    _fields_ = [("index", C.c_int64), ("chunk", C.c_uint32), ("seqno", C.c_uint32), ("pass_", C.c_uint8),
                ("kind", C.c_uint8), ("newc", C.c_uint8), ("oldc", C.c_uint8), ("rep", C.c_uint32),
                ("aux_off", C.c_uint32), ("aux_len", C.c_uint32)]


assert C.sizeof(FixRec) == 32


class KmerRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("n_kmers", C.c_uint64), ("n_absent", C.c_uint64), ("seq", C.c_uint32), ("min_count", C.c_uint32)]


assert C.sizeof(KmerRun) == 32


class CopyRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("n_kmers", C.c_uint64), ("sum_reads", C.c_uint64), ("sum_asm", C.c_uint64), ("seq", C.c_uint32), ("kind", C.c_uint32)]


assert C.sizeof(CopyRun) == 40


class PairRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("n_kmers", C.c_uint64), ("sum_reads", C.c_uint64), ("seq", C.c_uint32), ("kind", C.c_uint32)]


assert C.sizeof(PairRun) == 32


class DupRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("mate_start", C.c_int64), ("n_kmers", C.c_uint64), ("sum_reads", C.c_uint64), ("n_deficit", C.c_uint64),
                ("seq", C.c_uint32), ("mate_seq", C.c_uint32), ("strand", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(DupRun) == 56


class HapRun(C.Structure):
    _fields_ = [("start", C.c_int64), ("n_kmers", C.c_uint64), ("seq", C.c_uint32), ("kind", C.c_uint32)]


assert C.sizeof(HapRun) == 24


class Variant(C.Structure):
    _fields_ = [("pos", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("alt_min", C.c_uint32), ("ref", C.c_uint8), ("alt", C.c_uint8),
                ("kind", C.c_uint8), ("pad", C.c_uint8)]


assert C.sizeof(Variant) == 24


class Indel(C.Structure):
    _fields_ = [("pos", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("alt_min", C.c_uint32), ("len", C.c_uint16), ("type", C.c_uint8),
                ("base", C.c_uint8), ("kind", C.c_uint8), ("pad", C.c_uint8 * 7)]


assert C.sizeof(Indel) == 32


class MixedIns(C.Structure):
    _fields_ = [("pos", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("alt_min", C.c_uint32), ("bases", C.c_uint32), ("len", C.c_uint16),
                ("kind", C.c_uint8), ("pad", C.c_uint8 * 5)]


assert C.sizeof(MixedIns) == 32


class Compound(C.Structure):
    _fields_ = [("pos", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("alt_min", C.c_uint32), ("ref_len", C.c_uint32), ("bases", C.c_uint64 * 2),
                ("len", C.c_uint16), ("pad", C.c_uint8 * 6)]


assert C.sizeof(Compound) == 48


class HetCluster(C.Structure):
    _fields_ = Compound._fields_


assert C.sizeof(HetCluster) == 48


class Edit(C.Structure):
    _fields_ = [("pos", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("alt_min", C.c_uint32), ("ref_len", C.c_uint32), ("bases", C.c_uint64 * 2),
                ("len", C.c_uint16), ("source", C.c_uint8), ("round", C.c_uint8), ("pad", C.c_uint8 * 4)]


assert C.sizeof(Edit) == 48


class RepairRound(C.Structure):
    _fields_ = [("records", C.c_uint64), ("accepted", C.c_uint64), ("conflicts", C.c_uint64), ("ambiguous", C.c_uint64), ("unreliable_before", C.c_uint64),
                ("unreliable_after", C.c_uint64)]


assert C.sizeof(RepairRound) == 48


class GapSite(C.Structure):
    _fields_ = [("a", C.c_int64), ("q", C.c_int64), ("seq", C.c_uint32), ("ref_min", C.c_uint32), ("n_records", C.c_uint32), ("levels", C.c_uint32),
                ("trim_left", C.c_uint32), ("trim_right", C.c_uint32), ("kind", C.c_uint8), ("status", C.c_uint8), ("pad", C.c_uint8 * 6)]


assert C.sizeof(GapSite) == 48


class GapFill(C.Structure):
    _fields_ = [("pos", C.c_int64), ("bases_off", C.c_uint64), ("seq", C.c_uint32), ("ref_len", C.c_uint32), ("len", C.c_uint32), ("alt_min", C.c_uint32)]


assert C.sizeof(GapFill) == 32

# every symbol include/jasper_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "jasper_last_error": (C.c_char_p, []),
    "jasper_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "jasper_request_cancel": (C.c_int, [C.c_int]),
    "jasper_device_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_table_create": (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "jasper_table_load_jf": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "jasper_table_destroy": (None, [_P]),
    "jasper_table_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_table_sync": (C.c_int, [_P]),
    "jasper_table_clear": (C.c_int, [_P]),
    "jasper_count_bases": (C.c_int, [_P, C.c_char_p, C.c_uint64]),
    "jasper_count_bases_device": (C.c_int, [_P, _P, C.c_uint64]),
    "jasper_count_reads_text": (C.c_int, [_P, C.c_char_p, C.c_uint64]),
    "jasper_count_reads_files": (C.c_int, [_P, C.POINTER(C.c_char_p), C.c_int]),
    "jasper_count_reads_file_ranges": (C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "jasper_table_load_jf_part": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_table_write_jf": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_char_p), C.c_int]),
    "jasper_debug_mix": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "jasper_last_ingest": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_last_inflate": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_histogram_part": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "jasper_histogram_is_fused": (C.c_int, [_P]),
    "jasper_histogram": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_lookup": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64), C.c_uint64, C.POINTER(C.c_uint32)]),
    "jasper_table_export": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_table_import": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint64]),
    "jasper_table_export_device": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(_P)]),
    "jasper_table_import_device": (C.c_int, [_P, _P, C.c_uint64]),
    "jasper_table_export_to": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "jasper_device_free": (C.c_int, [_P, _P]),
    "jasper_table_export_packed": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32]),
    "jasper_table_import_packed": (C.c_int, [_P, _P, C.c_uint64, C.c_int]),
    "jasper_table_import_packed_multi": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64), C.c_uint32]),
    "jasper_table_reserve": (C.c_int, [_P, C.c_uint64]),
    "jasper_table_fit": (C.c_int, [_P, C.c_double]),
    "jasper_read_feed_start": (C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "jasper_read_feed_next": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "jasper_read_feed_release": (C.c_int, [_P]),
    "jasper_count_exchange_plan": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "jasper_count_exchange_scan": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "jasper_count_exchange_partition": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P, _P, C.c_uint64]),
    "jasper_count_exchange_dedupe": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "jasper_count_exchange_insert": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_int, C.c_uint32, C.c_int]),
    "jasper_table_export_owner": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "jasper_table_export_file_ranges": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_table_write_jf_piece": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "jasper_table_ipc_handle": (C.c_int, [_P, _P]),
    "jasper_table_attach_ipc": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32]),
    "jasper_table_attach_tables": (C.c_int, [_P, C.POINTER(_P), C.c_uint32, C.c_uint32]),
    "jasper_table_detach": (C.c_int, [_P]),
    "jasper_ipc_probe": (C.c_int, [C.c_int, _P, C.c_uint32, C.c_uint32]),
    "jasper_table_release_retired": (C.c_int, [_P]),
    "jasper_inflate_file": (C.c_int, [C.c_char_p, C.c_int, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "jasper_inflate_file_device": (C.c_int, [C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_owner_of": (C.c_uint32, [C.c_uint64, C.c_uint64, C.c_uint32]),
    "jasper_polish_batch": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_result_num_chunks": (C.c_int, [_P]),
    "jasper_polish_batch_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_result_seq": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "jasper_result_seq_len": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "jasper_result_seq_device": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "jasper_result_records": (C.c_int, [_P, C.POINTER(C.POINTER(FixRec)), C.POINTER(C.c_uint64)]),
    "jasper_result_aux": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "jasper_result_qv": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "jasper_result_qv_chunk": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "jasper_result_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_result_seconds": (C.c_double, [_P]),
    "jasper_result_segments": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_polish_cut_geometry": (C.c_int, [C.c_int, C.POINTER(C.c_int64)]),
    "jasper_result_retried": (C.c_int, [_P]),
    "jasper_result_free": (None, [_P]),
    "jasper_kmer_report": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.POINTER(_P)]),
    "jasper_kmer_report_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.POINTER(_P)]),
    "jasper_report_tile_windows": (C.c_int, []),
    "jasper_report_num_seqs": (C.c_int, [_P]),
    "jasper_report_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_report_runs": (C.c_int, [_P, C.POINTER(C.POINTER(KmerRun)), C.POINTER(C.c_uint64)]),
    "jasper_report_seconds": (C.c_double, [_P]),
    "jasper_report_retried": (C.c_int, [_P]),
    "jasper_report_free": (None, [_P]),
    "jasper_spectrum_rows": (C.c_int, []),
    "jasper_table_spectrum": (C.c_int, [_P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_copy_report": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_copy_report_device": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_copyrep_num_seqs": (C.c_int, [_P]),
    "jasper_copyrep_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_copyrep_runs": (C.c_int, [_P, C.POINTER(C.POINTER(CopyRun)), C.POINTER(C.c_uint64)]),
    "jasper_copyrep_seconds": (C.c_double, [_P]),
    "jasper_copyrep_retried": (C.c_int, [_P]),
    "jasper_copyrep_free": (None, [_P]),
    "jasper_table_spectrum_pair": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_pair_scan": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.POINTER(_P)]),
    "jasper_pairscan_num_seqs": (C.c_int, [_P]),
    "jasper_pairscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_pairscan_runs": (C.c_int, [_P, C.POINTER(C.POINTER(PairRun)), C.POINTER(C.c_uint64)]),
    "jasper_pairscan_seconds": (C.c_double, [_P]),
    "jasper_pairscan_retried": (C.c_int, [_P]),
    "jasper_pairscan_free": (None, [_P]),
    "jasper_dup_map": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_dup_map_device": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_dupmap_num_seqs": (C.c_int, [_P]),
    "jasper_dupmap_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_dupmap_runs": (C.c_int, [_P, C.POINTER(C.POINTER(DupRun)), C.POINTER(C.c_uint64)]),
    "jasper_dupmap_seconds": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "jasper_dupmap_retried": (C.c_int, [_P]),
    "jasper_dupmap_free": (None, [_P]),
    "jasper_hapmer_scan": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_hapmer_scan_device": (C.c_int, [_P, _P, _P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "jasper_hapscan_num_seqs": (C.c_int, [_P]),
    "jasper_hapscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_hapscan_runs": (C.c_int, [_P, C.POINTER(C.POINTER(HapRun)), C.POINTER(C.c_uint64)]),
    "jasper_hapscan_seconds": (C.c_double, [_P]),
    "jasper_hapscan_retried": (C.c_int, [_P]),
    "jasper_hapscan_free": (None, [_P]),
    "jasper_hapmer_census": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_table_select": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_table_subtract": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_count_binned": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(C.c_uint32), C.c_int64, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_count_binned_device": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(C.c_uint32), C.c_int64, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_read_text_count": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.POINTER(_P), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_read_bins": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(C.c_double)]),
    "jasper_read_bins_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(C.c_double)]),
    "jasper_read_text_bins": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "jasper_read_text_fetch": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "jasper_gz_text_open": (C.c_int, [_P, C.c_char_p, C.POINTER(_P)]),
    "jasper_gz_text_close": (None, [_P]),
    "jasper_gz_text_bins": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "jasper_gz_text_copy": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "jasper_gz_text_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_route_text": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "jasper_gz_text_route": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_double)]),
    "jasper_deflate_bound": (C.c_int64, [C.c_int64]),
    "jasper_deflate_bgzf": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_route_text_gz": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_gz_text_route_gz": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "jasper_variant_scan": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.POINTER(_P)]),
    "jasper_variant_scan_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.POINTER(_P)]),
    "jasper_varscan_num_seqs": (C.c_int, [_P]),
    "jasper_varscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_varscan_records": (C.c_int, [_P, C.POINTER(C.POINTER(Variant)), C.POINTER(C.c_uint64)]),
    "jasper_varscan_candidates": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_varscan_seconds": (C.c_double, [_P]),
    "jasper_varscan_retried": (C.c_int, [_P]),
    "jasper_varscan_free": (None, [_P]),
    "jasper_indel_scan": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_indel_scan_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_indelscan_num_seqs": (C.c_int, [_P]),
    "jasper_indelscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_records": (C.c_int, [_P, C.POINTER(C.POINTER(Indel)), C.POINTER(C.c_uint64)]),
    "jasper_indelscan_variants": (_P, [_P]),
    "jasper_indelscan_seconds": (C.c_double, [_P]),
    "jasper_indelscan_check_seconds": (C.c_double, [_P]),
    "jasper_indelscan_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_retried": (C.c_int, [_P]),
    "jasper_indelscan_free": (None, [_P]),
    "jasper_indel_scan_mixed": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_indel_scan_mixed_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_indelscan_mixed_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_mixed_records": (C.c_int, [_P, C.POINTER(C.POINTER(MixedIns)), C.POINTER(C.c_uint64)]),
    "jasper_indelscan_mixed_seconds": (C.c_double, [_P]),
    "jasper_indelscan_mixed_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_mixed_retried": (C.c_int, [_P]),
    "jasper_indel_front": (C.c_int, []),
    "jasper_indel_scan_clusters": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_indel_scan_clusters_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_indelscan_cluster_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_cluster_records": (C.c_int, [_P, C.POINTER(C.POINTER(HetCluster)), C.POINTER(C.c_uint64)]),
    "jasper_indelscan_cluster_seconds": (C.c_double, [_P]),
    "jasper_indelscan_cluster_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_indelscan_cluster_retried": (C.c_int, [_P]),
    "jasper_compound_scan": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_compound_scan_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.POINTER(_P)]),
    "jasper_compscan_num_seqs": (C.c_int, [_P]),
    "jasper_compscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_compscan_records": (C.c_int, [_P, C.POINTER(C.POINTER(Compound)), C.POINTER(C.c_uint64)]),
    "jasper_compscan_report": (_P, [_P]),
    "jasper_compscan_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_compscan_seconds": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "jasper_compscan_retried": (C.c_int, [_P]),
    "jasper_compound_front": (C.c_int, []),
    "jasper_compscan_free": (None, [_P]),
    "jasper_repair": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_repair_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_apply_edits": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _P, C.c_uint64, C.POINTER(_P)]),
    "jasper_apply_edits_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), _P, C.c_uint64, C.POINTER(_P)]),
    "jasper_repair_tile_bytes": (C.c_int, []),
    "jasper_repaired_num_seqs": (C.c_int, [_P]),
    "jasper_repaired_seq": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "jasper_repaired_edits": (C.c_int, [_P, C.POINTER(C.POINTER(Edit)), C.POINTER(C.c_uint64)]),
    "jasper_repaired_rounds": (C.c_int, [_P, C.POINTER(C.POINTER(RepairRound)), C.POINTER(C.c_uint64)]),
    "jasper_repaired_before": (_P, [_P]),
    "jasper_repaired_after": (_P, [_P]),
    "jasper_repaired_seconds": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "jasper_repaired_free": (None, [_P]),
    "jasper_gap_scan": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int64, C.c_int, C.POINTER(_P)]),
    "jasper_gap_scan_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int64, C.c_int, C.POINTER(_P)]),
    "jasper_gap_search": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.c_int, _P, C.c_uint64, C.POINTER(_P)]),
    "jasper_gap_search_device": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.c_uint32, C.c_int, _P, C.c_uint64, C.POINTER(_P)]),
    "jasper_gapscan_num_seqs": (C.c_int, [_P]),
    "jasper_gapscan_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "jasper_gapscan_sites": (C.c_int, [_P, C.POINTER(C.POINTER(GapSite)), C.POINTER(C.c_uint64)]),
    "jasper_gapscan_records": (C.c_int, [_P, C.POINTER(C.POINTER(GapFill)), C.POINTER(C.c_uint64)]),
    "jasper_gapscan_bases": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "jasper_gapscan_report": (_P, [_P]),
    "jasper_gapscan_seconds": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "jasper_gapscan_lookups": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "jasper_gapscan_retried": (C.c_int, [_P]),
    "jasper_gap_front": (C.c_int, []),
    "jasper_gap_max_records": (C.c_int, []),
    "jasper_gap_max_len": (C.c_int, []),
    "jasper_gapscan_free": (None, [_P]),
    "jasper_asm_open": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "jasper_asm_close": (None, [_P]),
    "jasper_asm_info": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_asm_contig": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_asm_split": (C.c_int, [_P, C.c_uint64, C.c_char_p, _P, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jasper_asm_split_wait": (C.c_int, [_P]),
    "jasper_asm_chunks": (C.c_int, [_P, _P, _P, _P, _P]),
    "jasper_asm_file_bytes": (C.c_int, [_P, _P]),
    "jasper_asm_chunk_text": (C.c_int, [_P, C.c_uint64, C.c_int, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "jasper_asm_polish": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "jasper_asm_pin": (C.c_int, [_P, C.c_int]),
    "jasper_asm_take": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "jasper_asm_put": (C.c_int, [_P, C.c_uint64, C.c_char_p, C.c_uint64]),
    "jasper_asm_write_fixed": (C.c_int, [_P, _P, C.POINTER(C.c_char_p), C.c_uint32, C.c_int]),
    "jasper_asm_polished_lens": (C.c_int, [_P, _P, _P]),
    "jasper_asm_join": (C.c_int, [_P, C.c_char_p, _P, C.c_int, C.c_int]),
    "jasper_merge_fix_csvs": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p]),
    "jasper_last_count_timing": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "jasper_last_count_stages": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
}

_lib = None


class JasperHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libjasper_hip: %s (code %d)" % (msg, code))
        self.code = code


def _share_hip_runtime_with_torch():
    """One process must use ONE HIP/HSA runtime. PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64;
    if libjasper_hip.so pulled in /opt/rocm's copies first, a later `import torch` finds "No HIP GPUs" (the second
    HSA runtime cannot open the device). So when torch is installed but not imported yet, load ITS runtime first;
    libjasper_hip.so's NEEDED libamdhip64.so.7 then resolves to the already-loaded copy. Without torch the system
    ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """load libjasper_hip.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run `make -C jasper_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise JasperHipError(rc, lib().jasper_last_error().decode(errors="replace"))


def kernel_source_digest():
    """sha256 over the native sources (jasper_amd/csrc/*.hip|hpp|cpp, include/*.h), file names and contents in sorted order:
    what a set of hardware counters under profiles/ was taken from.  bench.py cites committed counters only when this digest is
    the one stored with them (tools/summarize_prof.py) -- counters of other kernels are not evidence."""
    import glob
    import hashlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(root, "jasper_amd", "csrc", "*.h*")) + glob.glob(os.path.join(root, "jasper_amd", "csrc", "*.cpp")) +
                   glob.glob(os.path.join(root, "include", "*.h")))
    for fn in files:
        h.update(os.path.basename(fn).encode() + b"\0")
        with open(fn, "rb") as f:
            h.update(f.read())
    return h.hexdigest()
