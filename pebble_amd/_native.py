"""ctypes binding of the C-ABI in include/pebble_amd.h (libpebble_amd.so).

The shared library is built in-tree by pebble_amd.build (hipcc, gfx950) and is
the only implementation of the decode path: there is no CPU fallback.  Loading
fails loudly when the library is missing.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PBL_LIB selects the diagnostic (phase-stamp) build for scripts/pipe_stamps.py
LIB_PATH = os.environ.get("PBL_LIB") or os.path.join(_HERE, "libpebble_amd.so")

# status codes (include/pebble_amd.h)
PBL_OK = 0
PBL_CORRUPT_NO_RESTARTS = 1
PBL_CORRUPT_FIRST_KEY = 2
PBL_CORRUPT_BOUNDS = 3
PBL_CORRUPT_COLBLK_HEADER = 4
PBL_UNSUPPORTED = 5
PBL_OVERFLOW = 6
PBL_INVALID_ARG = 7
PBL_DEVICE_ERROR = 8
PBL_TIMEOUT = 9
PBL_CORRUPT_CHECKSUM = 10
PBL_CORRUPT_COMPRESSION = 11
PBL_CORRUPT_FOOTER = 12
PBL_CORRUPT_INDEX = 13
PBL_CORRUPT_VALUE_HANDLE = 14
PBL_CORRUPT_FILTER = 15
STATUS_NAMES = {
    0: "OK", 1: "CORRUPT_NO_RESTARTS", 2: "CORRUPT_FIRST_KEY", 3: "CORRUPT_BOUNDS",
    4: "CORRUPT_COLBLK_HEADER", 5: "UNSUPPORTED", 6: "OVERFLOW", 7: "INVALID_ARG",
    8: "DEVICE_ERROR", 9: "TIMEOUT", 10: "CORRUPT_CHECKSUM", 11: "CORRUPT_COMPRESSION",
    12: "CORRUPT_FOOTER", 13: "CORRUPT_INDEX", 14: "CORRUPT_VALUE_HANDLE",
    15: "CORRUPT_FILTER",
}
# TableFormat (footer magic, version)
PBL_TABLE_LEVELDB, PBL_TABLE_ROCKSDBV2 = 1, 2
PBL_TABLE_PEBBLEV1 = 3  # .. PBL_TABLE_PEBBLEV8 = 10
PBL_TABLE_PEBBLEV5, PBL_TABLE_PEBBLEV6, PBL_TABLE_PEBBLEV7 = 7, 8, 9
PBL_CHECKSUM_NONE, PBL_CHECKSUM_CRC32C, PBL_CHECKSUM_XXHASH, PBL_CHECKSUM_XXHASH64 = 0, 1, 2, 3
PBL_COMPRESSION_NONE, PBL_COMPRESSION_SNAPPY, PBL_COMPRESSION_ZSTD, PBL_COMPRESSION_MINLZ = 0, 1, 7, 8

ABI_VERSION = 9  # include/pebble_amd.h PBL_ABI_VERSION
PBL_LONGKEY_WGS = 32  # key spill slots of pbl_workspace_bytes_for

PBL_FMT_ROW = 0
PBL_FMT_COL_DEFAULT = 1
PBL_FMT_COL_CRDB1 = 2

PBL_ROW_VALUE_PREFIX = 0x1
PBL_ROW_NO_VALUER = 0x2
PBL_ROW_RAW_KEYS = 0x4
PBL_BATCH_VARLEN = 0x100
PBL_ROW_HIDE_OBSOLETE = 0x8
PBL_COL_TIERING = 0x10
PBL_KERNEL_SINGLE = 0x200
PBL_KERNEL_PIPE = 0x400
PBL_KERNEL_POOL = 0x4000
PBL_PHYS_MINLZ_NATIVE = 0x1

PBL_KV_RESTART = 0x01
PBL_KV_RESTART_SAMEPFX = 0x02
PBL_KV_OBSOLETE = 0x04
PBL_KV_INVALID_KEY = 0x08
PBL_KV_VALBLK_HANDLE = 0x10
PBL_KV_BLOB_HANDLE = 0x20
PBL_KV_PREFIX_CHANGED = 0x40

_vp = ctypes.c_void_p
_u8p = ctypes.POINTER(ctypes.c_uint8)


class BlockBatchC(ctypes.Structure):
    _fields_ = [
        ("blocks", _vp), ("block_off", _vp), ("block_len", _vp),
        ("n_blocks", ctypes.c_uint32), ("format", ctypes.c_uint32),
        ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("block_format", _vp), ("synthetic_seq_num", ctypes.c_uint64),
    ]


class ColGenConfigC(ctypes.Structure):
    _fields_ = [
        ("seed", ctypes.c_uint64), ("alphabet_len", ctypes.c_uint32),
        ("prefix_len_shared", ctypes.c_uint32), ("roach_key_len", ctypes.c_uint32),
        ("avg_keys_per_prefix", ctypes.c_uint32), ("base_wall_time", ctypes.c_uint64),
        ("pct_logical", ctypes.c_uint32), ("value_len", ctypes.c_uint32),
        ("obsolete_every", ctypes.c_uint32), ("tiering", ctypes.c_uint32),
        ("first_block", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class ZipfConfigC(ctypes.Structure):
    _fields_ = [
        ("seed", ctypes.c_uint64), ("key_min", ctypes.c_uint32), ("key_max", ctypes.c_uint32),
        ("val_min", ctypes.c_uint32), ("val_max", ctypes.c_uint32), ("s", ctypes.c_double),
        ("block_size", ctypes.c_uint32), ("restart_interval", ctypes.c_int32),
        ("first_block", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class TotalsC(ctypes.Structure):
    _fields_ = [
        ("n_kv", ctypes.c_uint64), ("key_bytes", ctypes.c_uint64),
        ("val_bytes", ctypes.c_uint64), ("n_restarts", ctypes.c_uint64),
        ("status_mask", ctypes.c_uint32), ("n_bad_blocks", ctypes.c_uint32),
        ("n_slow_blocks", ctypes.c_uint32), ("pad", ctypes.c_uint32),
    ]


class DecodeOutC(ctypes.Structure):
    _fields_ = [
        ("trailer", _vp), ("kv_flags", _vp), ("entry_off", _vp),
        ("key_off", _vp), ("val_off", _vp), ("key_bytes", _vp), ("val_bytes", _vp),
        ("restarts", _vp), ("blk_kv_base", _vp), ("blk_key_base", _vp),
        ("blk_val_base", _vp), ("blk_rst_base", _vp), ("blk_status", _vp),
        ("totals", _vp),
        ("kv_cap", ctypes.c_uint64), ("key_cap", ctypes.c_uint64),
        ("val_cap", ctypes.c_uint64), ("rst_cap", ctypes.c_uint64),
        ("workspace", _vp), ("workspace_bytes", ctypes.c_uint64),
        ("tiering_span_id", _vp), ("tiering_attr", _vp),
    ]


PBL_SPLIT_WHOLE, PBL_SPLIT_TESTKEYS, PBL_SPLIT_CRDB = 0, 1, 2


class PhysBatchC(ctypes.Structure):
    _fields_ = [("bytes", _vp), ("block_off", _vp), ("block_len", _vp), ("n_blocks", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class FooterC(ctypes.Structure):
    _fields_ = [
        ("table_format", ctypes.c_uint32), ("checksum_type", ctypes.c_uint32),
        ("metaindex_off", ctypes.c_uint64), ("metaindex_len", ctypes.c_uint64),
        ("index_off", ctypes.c_uint64), ("index_len", ctypes.c_uint64),
        ("footer_off", ctypes.c_uint64), ("footer_len", ctypes.c_uint64),
        ("attributes", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class IndexOutC(ctypes.Structure):
    _fields_ = [("handle_off", _vp), ("handle_len", _vp), ("props_off", _vp), ("props_len", _vp),
                ("blk_base", _vp), ("blk_status", _vp), ("cap", ctypes.c_uint64)]


class KvOutC(ctypes.Structure):
    _fields_ = [("key_off", _vp), ("key_len", _vp), ("val_off", _vp), ("val_len", _vp), ("blk_base", _vp),
                ("blk_status", _vp), ("cap", ctypes.c_uint64)]


class ValueOutC(ctypes.Structure):
    _fields_ = [("val_off", _vp), ("val_bytes", _vp), ("blk_val_base", _vp), ("blk_status", _vp),
                ("val_cap", ctypes.c_uint64)]


class TransformsC(ctypes.Structure):
    _fields_ = [
        ("synthetic_seq_num", ctypes.c_uint64), ("hide_obsolete_points", ctypes.c_uint32),
        ("split", ctypes.c_uint32), ("prefix", _vp), ("suffix", _vp),
        ("prefix_len", ctypes.c_uint32), ("suffix_len", ctypes.c_uint32),
        ("blocks", ctypes.POINTER(BlockBatchC)),
    ]


class KvC(ctypes.Structure):  # pbl_kv (base.InternalKV over the decoded arrays)
    _fields_ = [("user_key", _vp), ("user_key_len", ctypes.c_uint64), ("trailer", ctypes.c_uint64),
                ("value", _vp), ("value_len", ctypes.c_uint64), ("kv_flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class KvMetaC(ctypes.Structure):  # pbl_kv_meta (base.KVMeta)
    _fields_ = [("tiering_span_id", ctypes.c_uint64), ("tiering_attribute", ctypes.c_uint64)]


PBL_CMP_DEFAULT, PBL_CMP_TESTKEYS, PBL_CMP_CRDB = 0, 1, 2
_kvp = ctypes.POINTER(KvC)
_u8p = ctypes.c_char_p

# batched seeks (pbl_seek_batch)
PBL_SEEK_GE, PBL_SEEK_LT = 0, 1
PBL_SEEK_NONE = (1 << 64) - 1
PBL_SEEK_EXACT, PBL_SEEK_SAME_PREFIX, PBL_SEEK_BAD_BLOCK = 0x1, 0x2, 0x4


class SeekQueriesC(ctypes.Structure):  # pbl_seek_queries
    _fields_ = [("key_bytes", _vp), ("key_off", _vp), ("block", _vp), ("n", ctypes.c_uint32),
                ("comparer", ctypes.c_uint32), ("op", ctypes.c_uint32), ("hide_obsolete_points", ctypes.c_uint32)]


class SeekOutC(ctypes.Structure):  # pbl_seek_out
    _fields_ = [("kv", _vp), ("block", _vp), ("flags", _vp)]


# batched bounded scans (pbl_scan_batch)
PBL_SCAN_NO_UPPER = 0x1  # pbl_scan_queries.flags[i]
PBL_SCAN_SIZED = 0x1     # pbl_scan_batch flags


class ScanQueriesC(ctypes.Structure):  # pbl_scan_queries
    _fields_ = [("lower_bytes", _vp), ("lower_off", _vp), ("upper_bytes", _vp), ("upper_off", _vp),
                ("flags", _vp), ("block", _vp), ("n", ctypes.c_uint32), ("comparer", ctypes.c_uint32),
                ("hide_obsolete_points", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ScanOutC(ctypes.Structure):  # pbl_scan_out
    _fields_ = [("result", DecodeOutC), ("range", _vp), ("src_kv", _vp)]


# batched k-way merge (pbl_merge_batch)
PBL_MERGE_MAX_RUNS = 16
PBL_MERGE_SIZED = 0x1  # pbl_merge_batch flags


class MergeRunsC(ctypes.Structure):  # pbl_merge_runs
    _fields_ = [("runs", ctypes.POINTER(DecodeOutC)), ("n_runs", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32),
                ("comparer", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_kv_total", ctypes.c_uint64)]


class MergeOutC(ctypes.Structure):  # pbl_merge_out
    _fields_ = [("result", DecodeOutC), ("src_run", _vp), ("src_kv", _vp)]


# batched snapshot-visible view (pbl_visible_batch)
PBL_SEQNUM_MAX = (1 << 56) - 1
PBL_VISIBLE_SIZED = 0x1           # pbl_visible_batch flags
PBL_VISIBLE_KEEP_OPERANDS = 0x2   # pbl_visible_size / pbl_visible_batch / pbl_visible_batch_host flags


class VisibleInC(ctypes.Structure):  # pbl_visible_in
    _fields_ = [("batch", DecodeOutC), ("n_blocks", ctypes.c_uint32), ("comparer", ctypes.c_uint32),
                ("n_kv", ctypes.c_uint64), ("snapshot", ctypes.c_uint64)]


class VisibleOutC(ctypes.Structure):  # pbl_visible_out
    _fields_ = [("result", DecodeOutC), ("src_kv", _vp), ("n_src", _vp)]


# compaction view (pbl_compact_batch)
PBL_COMPACT_SIZED = 0x1              # pbl_compact_batch flags
PBL_COMPACT_ELIDE_TOMBSTONES = 0x2   # pbl_compact_size / pbl_compact_batch / pbl_compact_batch_host flags
PBL_COMPACT_BOTTOMMOST = 0x4


class CompactInC(ctypes.Structure):  # pbl_compact_in
    _fields_ = [("batch", DecodeOutC), ("n_blocks", ctypes.c_uint32), ("comparer", ctypes.c_uint32),
                ("n_kv", ctypes.c_uint64), ("snapshots", _vp), ("n_snapshots", ctypes.c_uint64)]


class CompactOutC(ctypes.Structure):  # pbl_compact_out
    _fields_ = [("result", DecodeOutC), ("src_kv", _vp), ("n_src", _vp), ("pinned", _vp), ("n_missized", _vp),
                ("n_ineffectual", _vp), ("n_nondeterministic", _vp)]


# row-block encoder (pbl_rowenc_batch)
PBL_ENC_VALUE_PREFIX, PBL_ENC_OBSOLETE, PBL_ENC_LOWEST_LEVEL = 0x1, 0x2, 0x4  # pbl_rowenc_opts.flags
PBL_ROWENC_SIZED = 0x1  # pbl_rowenc_batch flags


class RowEncOptsC(ctypes.Structure):  # pbl_rowenc_opts
    _fields_ = [("restart_interval", ctypes.c_uint32), ("target_block_size", ctypes.c_uint32),
                ("block_size_threshold", ctypes.c_uint32), ("comparer", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class RowEncInC(ctypes.Structure):  # pbl_rowenc_in
    _fields_ = [("batch", DecodeOutC), ("n_streams", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("n_kv", ctypes.c_uint64)]


class RowEncTotalsC(ctypes.Structure):  # pbl_rowenc_totals
    _fields_ = [("n_blocks", ctypes.c_uint64), ("block_bytes", ctypes.c_uint64), ("n_restarts", ctypes.c_uint64),
                ("status_mask", ctypes.c_uint32), ("n_bad_streams", ctypes.c_uint32)]


class RowEncOutC(ctypes.Structure):  # pbl_rowenc_out
    _fields_ = [("blocks", _vp), ("block_off", _vp), ("block_len", _vp), ("block_stream", _vp),
                ("block_first_kv", _vp), ("block_n_kv", _vp), ("stream_block_base", _vp), ("stream_status", _vp),
                ("obsolete", _vp), ("totals", _vp), ("blocks_cap", ctypes.c_uint64), ("block_cap", ctypes.c_uint64)]


# range deletions in the read path (pbl_rangedel_set, pbl_rangedel_cover, the view's _rd entry points)
PBL_RANGEDEL_MAX_RUNS = 16
PBL_KIND_RANGEDEL = 15
PBL_RANGEDEL_ALL = 1 << 56  # a cover above every sequence number


class RangedelRunsC(ctypes.Structure):  # pbl_rangedel_runs
    _fields_ = [("runs", ctypes.POINTER(DecodeOutC)), ("n_kv", ctypes.POINTER(ctypes.c_uint64)),
                ("n_runs", ctypes.c_uint32), ("comparer", ctypes.c_uint32), ("snapshot", ctypes.c_uint64),
                ("level", ctypes.POINTER(ctypes.c_uint8))]


# columnar keyspan blocks (pbl_keyspan_decode)
class KeyspanExtraC(ctypes.Structure):  # pbl_keyspan_extra
    _fields_ = [("span", _vp), ("suffix_off", _vp), ("value_off", _vp), ("suffix_bytes", _vp), ("value_bytes", _vp),
                ("blk_suffix_base", _vp), ("blk_value_base", _vp), ("suffix_cap", ctypes.c_uint64),
                ("value_cap", ctypes.c_uint64)]


# range keys in the read path (pbl_rangekey_set_host, pbl_rangekey_mask)
PBL_KIND_RANGEKEYDEL, PBL_KIND_RANGEKEYUNSET, PBL_KIND_RANGEKEYSET = 19, 20, 21


class RangekeyRunsC(ctypes.Structure):  # pbl_rangekey_runs
    _fields_ = [("runs", ctypes.POINTER(DecodeOutC)), ("extras", ctypes.POINTER(KeyspanExtraC)),
                ("n_kv", ctypes.POINTER(ctypes.c_uint64)), ("n_runs", ctypes.c_uint32), ("comparer", ctypes.c_uint32),
                ("snapshot", ctypes.c_uint64)]


# table bloom filters (pbl_filter_probe, pbl_seek_prefix_batch)
PBL_FILTER_MAY, PBL_FILTER_BAD = 0x1, 0x2
PBL_SEEK_FILTERED = 0x8


class FilterSetC(ctypes.Structure):  # pbl_filter_set
    _fields_ = [("bytes", _vp), ("off", _vp), ("n_filters", ctypes.c_uint32)]


class FilterQueriesC(ctypes.Structure):  # pbl_filter_queries
    _fields_ = [("key_bytes", _vp), ("key_off", _vp), ("filter", _vp), ("n", ctypes.c_uint32),
                ("comparer", ctypes.c_uint32)]


class FilterOutC(ctypes.Structure):  # pbl_filter_out
    _fields_ = [("may", _vp), ("hash", _vp), ("flt_status", _vp)]


# Every symbol include/pebble_amd.h declares, with its ctypes signature.
SIGNATURES = {
    "pbl_data_iter_new": (_vp, []),
    "pbl_data_iter_free": (None, [_vp]),
    "pbl_data_iter_init": (ctypes.c_int, [_vp, ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_uint32]),
    "pbl_data_iter_first": (_kvp, [_vp]),
    "pbl_data_iter_last": (_kvp, [_vp]),
    "pbl_data_iter_next": (_kvp, [_vp]),
    "pbl_data_iter_prev": (_kvp, [_vp]),
    "pbl_data_iter_seek_ge": (_kvp, [_vp, _u8p, ctypes.c_uint64, ctypes.c_uint32]),
    "pbl_data_iter_seek_lt": (_kvp, [_vp, _u8p, ctypes.c_uint64, ctypes.c_uint32]),
    "pbl_data_iter_seek_prefix_ge": (_kvp, [_vp, _u8p, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.POINTER(ctypes.c_int)]),
    "pbl_data_iter_first_with_meta": (_kvp, [_vp, ctypes.POINTER(KvMetaC)]),
    "pbl_data_iter_next_with_meta": (_kvp, [_vp, ctypes.POINTER(KvMetaC)]),
    "pbl_data_iter_seek_ge_with_meta": (_kvp, [_vp, _u8p, ctypes.c_uint64, ctypes.c_uint32,
                                               ctypes.POINTER(KvMetaC)]),
    "pbl_data_iter_next_with_same_prefix": (_kvp, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "pbl_data_iter_next_prefix": (_kvp, [_vp, _u8p, ctypes.c_uint64]),
    "pbl_data_iter_is_lower_bound": (ctypes.c_int, [_vp, _u8p, ctypes.c_uint64]),
    "pbl_data_iter_valid": (ctypes.c_int, [_vp]),
    "pbl_data_iter_kv": (_kvp, [_vp]),
    "pbl_data_iter_invalidate": (None, [_vp]),
    "pbl_data_iter_is_data_invalidated": (ctypes.c_int, [_vp]),
    "pbl_key_compare": (ctypes.c_int, [ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, ctypes.c_uint64]),
    "pbl_key_split": (ctypes.c_uint64, [ctypes.c_uint32, _u8p, ctypes.c_uint64]),
    "pbl_seek_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32]),
    "pbl_seek_prepare": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint32, _vp,
                                        ctypes.c_uint64, _vp]),
    "pbl_seek_batch": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.POINTER(SeekQueriesC),
                                      ctypes.POINTER(SeekOutC), _vp, ctypes.c_uint64, _vp]),
    "pbl_seek_batch_host": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                           ctypes.POINTER(SeekQueriesC), ctypes.POINTER(SeekOutC)]),
    "pbl_seek_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_scan_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_scan_prepare": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                        ctypes.c_uint32, _vp, ctypes.c_uint64, _vp]),
    "pbl_scan_size": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint64,
                                     ctypes.POINTER(ScanQueriesC), ctypes.POINTER(ScanOutC), _vp, ctypes.c_uint64,
                                     _vp]),
    "pbl_scan_batch": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint64,
                                      ctypes.POINTER(ScanQueriesC), ctypes.POINTER(ScanOutC), _vp, ctypes.c_uint64,
                                      ctypes.c_uint32, _vp]),
    "pbl_scan_batch_host": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                           ctypes.POINTER(ScanQueriesC), ctypes.POINTER(ScanOutC)]),
    "pbl_scan_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_merge_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_merge_size": (ctypes.c_int, [ctypes.POINTER(MergeRunsC), ctypes.POINTER(MergeOutC), _vp, ctypes.c_uint64,
                                      _vp]),
    "pbl_merge_batch": (ctypes.c_int, [ctypes.POINTER(MergeRunsC), ctypes.POINTER(MergeOutC), _vp, ctypes.c_uint64,
                                       ctypes.c_uint32, _vp]),
    "pbl_merge_batch_host": (ctypes.c_int, [ctypes.POINTER(MergeRunsC), ctypes.POINTER(MergeOutC)]),
    "pbl_merge_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_visible_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_visible_size": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC), _vp, ctypes.c_uint64,
                                        ctypes.c_uint32, _vp]),
    "pbl_visible_batch": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC), _vp, ctypes.c_uint64,
                                         ctypes.c_uint32, _vp]),
    "pbl_visible_batch_host": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC),
                                              ctypes.c_uint32]),
    "pbl_visible_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_rangedel_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint64]),
    "pbl_rangedel_set": (ctypes.c_int, [ctypes.POINTER(RangedelRunsC), ctypes.POINTER(DecodeOutC), _vp, ctypes.c_uint64,
                                        _vp]),
    "pbl_rangedel_set_host": (ctypes.c_int, [ctypes.POINTER(RangedelRunsC), ctypes.POINTER(DecodeOutC)]),
    "pbl_rangedel_cover": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                          ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "pbl_rangedel_cover_host": (ctypes.c_int, [ctypes.POINTER(RangedelRunsC), ctypes.POINTER(DecodeOutC),
                                               ctypes.c_uint32, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "pbl_rangedel_cover_lv": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                             ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "pbl_rangedel_cover_host_lv": (ctypes.c_int, [ctypes.POINTER(RangedelRunsC), ctypes.POINTER(DecodeOutC),
                                                  ctypes.c_uint32, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "pbl_visible_size_rd": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC), _vp,
                                           ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "pbl_visible_batch_rd": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC), _vp,
                                            ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "pbl_visible_batch_host_rd": (ctypes.c_int, [ctypes.POINTER(VisibleInC), ctypes.POINTER(VisibleOutC),
                                                 ctypes.c_uint32, _vp]),
    "pbl_rangedel_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_keyspan_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_keyspan_size": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.c_uint64, ctypes.POINTER(DecodeOutC),
                                        ctypes.POINTER(KeyspanExtraC), _vp, ctypes.c_uint64, _vp]),
    "pbl_keyspan_decode": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.c_uint64, ctypes.POINTER(DecodeOutC),
                                          ctypes.POINTER(KeyspanExtraC), _vp, ctypes.c_uint64, _vp]),
    "pbl_keyspan_decode_host": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.POINTER(DecodeOutC),
                                               ctypes.POINTER(KeyspanExtraC)]),
    "pbl_keyspan_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_range_suffix_compare": (ctypes.c_int, [ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, ctypes.c_uint64]),
    "pbl_rangekey_set_host": (ctypes.c_int, [ctypes.POINTER(RangekeyRunsC), ctypes.POINTER(DecodeOutC),
                                             ctypes.POINTER(KeyspanExtraC)]),
    "pbl_rangekey_clip_host": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.POINTER(KeyspanExtraC),
                                              ctypes.POINTER(ScanQueriesC), ctypes.POINTER(DecodeOutC),
                                              ctypes.POINTER(KeyspanExtraC)]),
    "pbl_rangekey_mask": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.POINTER(KeyspanExtraC),
                                         ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                         _vp, ctypes.c_uint64, _vp, _vp]),
    "pbl_rangekey_mask_set_host": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.POINTER(KeyspanExtraC),
                                                  ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                                  ctypes.c_uint64, _vp]),
    "pbl_rangekey_mask_host": (ctypes.c_int, [ctypes.POINTER(RangekeyRunsC), ctypes.POINTER(DecodeOutC),
                                              ctypes.c_uint32, _u8p, ctypes.c_uint64, _vp,
                                              ctypes.POINTER(ctypes.c_uint32)]),
    "pbl_rangekey_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_filter_probe": (ctypes.c_int, [ctypes.POINTER(FilterSetC), ctypes.POINTER(FilterQueriesC),
                                        ctypes.POINTER(FilterOutC), _vp]),
    "pbl_filter_probe_host": (ctypes.c_int, [ctypes.POINTER(FilterSetC), ctypes.POINTER(FilterQueriesC),
                                             ctypes.POINTER(FilterOutC)]),
    "pbl_bloom_build_host": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                            ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "pbl_bloom_build_bound": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32]),
    "pbl_filter_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_seek_prefix_batch": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                             ctypes.POINTER(SeekQueriesC), _vp, ctypes.c_uint64,
                                             ctypes.POINTER(SeekOutC), _vp, ctypes.c_uint64, _vp]),
    "pbl_seek_prefix_batch_host": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32,
                                                  ctypes.POINTER(SeekQueriesC), _vp, ctypes.c_uint64,
                                                  ctypes.POINTER(SeekOutC)]),
    "pbl_compact_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_compact_size": (ctypes.c_int, [ctypes.POINTER(CompactInC), ctypes.POINTER(CompactOutC), _vp, ctypes.c_uint64,
                                        ctypes.c_uint32, _vp]),
    "pbl_compact_batch": (ctypes.c_int, [ctypes.POINTER(CompactInC), ctypes.POINTER(CompactOutC), _vp, ctypes.c_uint64,
                                         ctypes.c_uint32, _vp]),
    "pbl_compact_batch_host": (ctypes.c_int, [ctypes.POINTER(CompactInC), ctypes.POINTER(CompactOutC),
                                              ctypes.c_uint32]),
    "pbl_compact_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_rowenc_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint64]),
    "pbl_rowenc_size": (ctypes.c_int, [ctypes.POINTER(RowEncInC), ctypes.POINTER(RowEncOptsC),
                                       ctypes.POINTER(RowEncOutC), _vp, ctypes.c_uint64, _vp]),
    "pbl_rowenc_batch": (ctypes.c_int, [ctypes.POINTER(RowEncInC), ctypes.POINTER(RowEncOptsC),
                                        ctypes.POINTER(RowEncOutC), _vp, ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "pbl_rowenc_batch_host": (ctypes.c_int, [ctypes.POINTER(RowEncInC), ctypes.POINTER(RowEncOptsC),
                                             ctypes.POINTER(RowEncOutC)]),
    "pbl_rowenc_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_abi_version": (ctypes.c_int, []),
    "pbl_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32]),
    "pbl_workspace_bytes_for": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    "pbl_decode_batch": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.POINTER(DecodeOutC), _vp]),
    "pbl_size_batch": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.POINTER(DecodeOutC), _vp]),
    "pbl_struct_layout": (ctypes.c_size_t, [_vp, ctypes.c_size_t]),
    "pbl_transform_workspace_bytes": (ctypes.c_uint64, [ctypes.c_uint32]),
    "pbl_verify_checksums": (ctypes.c_int, [ctypes.POINTER(PhysBatchC), ctypes.c_uint32, _vp, _vp, _vp]),
    "pbl_decompressed_lengths": (ctypes.c_int, [ctypes.POINTER(PhysBatchC), _vp, _vp, _vp]),
    "pbl_decompress_blocks": (ctypes.c_int, [ctypes.POINTER(PhysBatchC), _vp, _vp, _vp, _vp, _vp, _vp]),
    "pbl_parse_footer": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(FooterC)]),
    "pbl_index_handles_row": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.POINTER(IndexOutC),
                                             _vp]),
    "pbl_index_handles_col": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.POINTER(IndexOutC), _vp]),
    "pbl_kv_blocks": (ctypes.c_int, [ctypes.POINTER(BlockBatchC), ctypes.POINTER(KvOutC), _vp]),
    "pbl_valblk_index": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "pbl_resolve_values": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.POINTER(BlockBatchC),
                                          ctypes.POINTER(ValueOutC), _vp]),
    "pbl_transform_batch": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.POINTER(TransformsC),
                                           ctypes.POINTER(DecodeOutC), _vp]),
    "pbl_rebase_blocks": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, ctypes.c_uint64,
                                         ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _vp]),
    "pbl_offset_concat": (ctypes.c_int, [ctypes.POINTER(DecodeOutC), ctypes.c_uint32, _vp, ctypes.c_uint32, _vp]),
    "pbl_rowblk_writer_new": (_vp, [ctypes.c_int]),
    "pbl_rowblk_writer_free": (None, [_vp]),
    "pbl_rowblk_writer_reset": (None, [_vp, ctypes.c_int]),
    "pbl_rowblk_writer_add": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64,
                                             ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.c_int64, ctypes.c_int, ctypes.c_uint8, ctypes.c_int]),
    "pbl_rowblk_writer_add_raw": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t,
                                                 ctypes.c_char_p, ctypes.c_size_t]),
    "pbl_rowblk_writer_estimated_size": (ctypes.c_size_t, [_vp]),
    "pbl_rowblk_writer_entry_count": (ctypes.c_size_t, [_vp]),
    "pbl_rowblk_writer_finish": (ctypes.c_size_t, [_vp, _vp, ctypes.c_size_t]),
    "pbl_gen_row_blocks": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                             _vp, _vp, _vp, ctypes.c_int]),
    "pbl_gen_row_blocks_obs": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                                 ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_int]),
    "pbl_colblk_writer_new": (_vp, [ctypes.c_uint32, ctypes.c_int]),
    "pbl_colblk_writer_free": (None, [_vp]),
    "pbl_colblk_writer_reset": (None, [_vp]),
    "pbl_colblk_writer_add": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64,
                                             ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                             ctypes.c_int]),
    "pbl_colblk_writer_set_tiering": (None, [_vp, ctypes.c_int]),
    "pbl_colblk_writer_add_meta": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64,
                                                  ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p,
                                                  ctypes.c_size_t]),
    "pbl_colblk_writer_rows": (ctypes.c_uint32, [_vp]),
    "pbl_colblk_writer_size": (ctypes.c_size_t, [_vp, ctypes.c_uint32]),
    "pbl_colblk_writer_finish": (ctypes.c_size_t, [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t]),
    "pbl_gen_col_blocks": (ctypes.c_uint64, [ctypes.POINTER(ColGenConfigC), ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_int]),
    "pbl_gen_zipf_blocks": (ctypes.c_uint64, [ctypes.POINTER(ZipfConfigC), ctypes.c_uint32, ctypes.c_uint32,
                                              _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_int]),
}

_lib = None
_gen_lib = None


def gen_lib() -> ctypes.CDLL:
    """The library for host-only work (synthetic generators, block writers):
    always the in-tree build, so that an A/B run of an older decoder build
    (PBL_LIB) generates exactly the same inputs."""
    global _gen_lib
    if not os.environ.get("PBL_LIB"):
        return lib()
    if _gen_lib is None:
        L = ctypes.CDLL(os.path.join(_HERE, "libpebble_amd.so"))
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _gen_lib = L
    return _gen_lib


def lib() -> ctypes.CDLL:
    """Load libpebble_amd.so (torch is imported first so that the HIP runtime it
    bundles is the one the library binds to: same SONAME, one runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the decode path.")
    try:
        import torch  # noqa: F401  (binds libamdhip64.so.7 first)
    except Exception:  # pragma: no cover - torch is always present in this image
        pass
    L = ctypes.CDLL(LIB_PATH)
    ab_build = bool(os.environ.get("PBL_LIB"))
    for name, (res, args) in SIGNATURES.items():
        if ab_build and not hasattr(L, name):
            continue  # an older A/B build (scripts/ab.sh): entry points it predates stay unbound
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.pbl_abi_version() != ABI_VERSION and not ab_build:
        raise RuntimeError("libpebble_amd.so ABI mismatch")
    _lib = L
    return L
