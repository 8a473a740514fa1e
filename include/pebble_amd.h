/*
 * pebble_amd.h — C-ABI of the MI355X-native Pebble SSTable data-block decoder.
 *
 * This is the drop-in boundary described in SURVEY.md §8(b).  A thin cgo shim
 * behind Pebble's `sstable/blockiter.Data` interface (or the Python host layer
 * in pebble_amd/) calls these entry points once per BATCH of data blocks; the
 * per-KV work runs in hand-written gfx950 HIP kernels.
 *
 * Reference interfaces replaced (paths relative to cockroachdb/pebble):
 *   pbl_decode_batch      rowblk.Iter.Init/First/Next  sstable/rowblk/rowblk_iter.go:241-276,1061-1087,1145-1201
 *                         colblk.DataBlockDecoder.Init sstable/colblk/data_block.go:1096-1109
 *                         colblk.DataBlockIter.Next    sstable/colblk/data_block.go:1662-1708
 *                         (driven by singleLevelIterator.loadDataBlock, sstable/reader_iter_single_lvl.go:485-547)
 *   pbl_rowblk_writer_*   rowblk.Writer                sstable/rowblk/rowblk_writer.go:48-320 (format producer)
 *   PBL_STATUS_*          base.CorruptionErrorf sites  sstable/rowblk/rowblk_iter.go:249-251,471-476;
 *                                                      sstable/colblk/data_block.go:1005-1009
 *
 * Conventions
 *   - Every pointer in pbl_block_batch / pbl_decode_out is a DEVICE pointer unless
 *     the field says otherwise.  The caller owns every buffer; the library never
 *     allocates or frees caller memory (mirrors block.BufferHandle ownership,
 *     sstable/blockiter/block_iter.go:76-81).
 *   - `stream` is a hipStream_t passed as void* (0 = legacy default stream).  All
 *     device entry points are stream-ordered and asynchronous; they never
 *     synchronise and are safe to capture into a hipGraph.
 *   - A launch runs on the device of its `stream` (hipStreamGetDevice), whatever
 *     the calling thread's current device.  The library is reentrant across
 *     streams and devices; its only process-wide state is a per-device cache of
 *     hardware properties (CU count, resident workgroups per kernel), written
 *     once.  Kernel choice depends only on the batch (format, flags), never on
 *     the environment.
 */
#ifndef PEBBLE_AMD_H
#define PEBBLE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBL_ABI_VERSION 9

/* ---- status codes (per block, and OR-ed as bit masks into totals) ---------- */
enum {
  PBL_OK = 0,
  PBL_CORRUPT_NO_RESTARTS = 1,   /* rowblk_iter.go:249-251 */
  PBL_CORRUPT_FIRST_KEY = 2,     /* rowblk_iter.go:429-434,471-476 */
  PBL_CORRUPT_BOUNDS = 3,        /* entry/column extends past the block */
  PBL_CORRUPT_COLBLK_HEADER = 4, /* data_block.go:1005-1009 (panic -> corruption) */
  PBL_UNSUPPORTED = 5,           /* legal but outside this build's limits.  For a
                                    row block: a key longer than 32768 bytes with no
                                    (or too small a) key spill slot in the workspace
                                    (pbl_workspace_bytes_for), or more than 4 GiB of
                                    key or value bytes in one block.  The block is
                                    not corrupt: decode it on the host. */
  PBL_OVERFLOW = 6,              /* an output capacity was too small: nothing written */
  PBL_INVALID_ARG = 7,
  PBL_DEVICE_ERROR = 8,
  PBL_TIMEOUT = 9,               /* in-kernel look-back spin bound hit (never expected) */
  PBL_CORRUPT_CHECKSUM = 10,     /* block.go:177-195 "checksum mismatch"        */
  PBL_CORRUPT_COMPRESSION = 11,  /* snappy.ErrCorrupt -> base.MarkCorruptionError (block.go:550-565) */
  PBL_CORRUPT_FOOTER = 12,       /* parseFooter's CorruptionErrorf sites (sstable/table.go:328-404) */
  PBL_CORRUPT_INDEX = 13,        /* DecodeHandleWithProperties "invalid block.Handle" (block/block.go:94-104) */
  PBL_CORRUPT_VALUE_HANDLE = 14, /* valblk handle/index entry out of bounds (valblk/valblk.go:370-393,
                                    valblk/reader.go:280-302) */
  PBL_CORRUPT_FILTER = 15        /* a bloom filter block whose trailer does not match its length
                                    (tablefilters/bloom/bits.go:100-102 panics there) */
};

/* ---- block formats ---------------------------------------------------------- */
enum {
  PBL_FMT_ROW = 0,          /* sstable/rowblk data block                          */
  PBL_FMT_COL_DEFAULT = 1,  /* colblk data block, colblk.DefaultKeySchema          */
  PBL_FMT_COL_CRDB1 = 2     /* colblk data block, cockroachkvs.KeySchema ("crdb1") */
};

/* batch flags */
#define PBL_ROW_VALUE_PREFIX 0x1u /* TableFormat >= Pebblev3: SET values carry a
                                     1-byte block.ValuePrefix (rowblk_iter.go:298-300) */
#define PBL_ROW_NO_VALUER 0x2u    /* iterator has no lazy valuer: strip the prefix
                                     byte even for handles (rowblk_iter.go:1195)   */
#define PBL_ROW_RAW_KEYS 0x4u     /* rowblk.RawIter semantics (rowblk_iter.go:1743-1794):
                                     keys are emitted whole, no trailer split, no
                                     first-key check; trailer[] = 0              */
#define PBL_ROW_HIDE_OBSOLETE 0x8u /* blockiter.Transforms.HideObsoletePoints fused into
                                     the decode (rowblk_iter.go:1168-1179; colblk
                                     data_block.go:1680-1697): KVs whose trailer has
                                     the obsolete bit (row) or whose isObsolete bit
                                     is set (colblk) are not emitted; every count and
                                     offset covers the visible KVs only, restart
                                     words are kept.  Row blocks ignore it with
                                     PBL_ROW_RAW_KEYS (a raw key has no trailer);
                                     colblk blocks always honour it.  Single-format
                                     and mixed (block_format) batches alike.  (The
                                     name is historical: it applies to colblk
                                     blocks too.)                                   */
#define PBL_COL_TIERING 0x10u     /* colblk blocks carry the Pebblev8 tiering columns
                                     (TableFormat.TieringColumnConfig, sstable/format.go:
                                     305-316: WithTieringColumns, data_block.go:594-601):
                                     the data columns tieringSpanID (Uint), tieringAttribute
                                     (Uint) and secondaryBlobHandle (RawBytes) follow
                                     isObsolete (data_block.go:514-525).  With it, every
                                     colblk KV's KVMeta -- what DataBlockIter.FirstWithMeta
                                     / NextWithMeta / SeekGEWithMeta return
                                     (data_block.go:1574-1641) -- is written to
                                     pbl_decode_out.tiering_span_id / tiering_attr when
                                     those are non-NULL, and the two Uint columns are
                                     decoded with DecodeColumn's checks (a block missing
                                     them, or failing them, is PBL_CORRUPT_COLBLK_HEADER:
                                     the reference panics in initTieringMetadata).
                                     Without it the meta arrays, when given, receive
                                     zeros (KVMeta{}: !SupportsTiering).  Row blocks
                                     always give zeros (rowblk.Iter has no meta columns;
                                     NextWithMeta on the row iterator returns KVMeta{}).
                                     Keys and values decode identically either way.   */
#define PBL_BATCH_VARLEN 0x100u   /* scheduling hint, no effect on results: block
                                     lengths vary widely (e.g. Zipf value sizes).
                                     colblk batches read more of each block's
                                     values from LDS; row batches take the
                                     two-pass form (lane-per-block size walk, bases
                                     scan, wave-per-block emit from LDS, no
                                     look-back) unless HideObsoletePoints or value
                                     prefixes need key bytes to size a block.  Set
                                     it for row batches of value-dominated blocks
                                     (few entries per block); blocks of many small
                                     KVs decode faster without it.  The caller
                                     knows the lengths on the host (block handles
                                     carry them); the Python layer also samples
                                     entry counts (batch.varlen_hint).             */
#define PBL_KERNEL_SINGLE 0x200u  /* A/B measurement, no effect on results: colblk
                                     batches on the one-block-per-workgroup kernel
                                     instead of the two-pass wave form (row
                                     batches ignore it)                            */
#define PBL_KERNEL_PIPE 0x400u    /* A/B measurement, no effect on results: colblk
                                     batches on the persistent pipeline instead of
                                     the two-pass wave form (row batches ignore
                                     it)                                           */
/* 0x800u, 0x1000u, 0x2000u, 0x8000u: retired A/B kernels (one-wave-per-block
   flat, run-major, HBM-walking and block-resident row kernels; removed, the
   bits are ignored)                                                            */
#define PBL_KERNEL_POOL 0x4000u   /* A/B measurement, no effect on results: row
                                     batches on the staging-pool kernel
                                     (rowblk_pool.hip.h, the default without
                                     PBL_BATCH_VARLEN) even with PBL_BATCH_VARLEN  */

/* per-KV flag byte (kv_flags[]) */
#define PBL_KV_RESTART 0x01u       /* entry offset is a restart point            */
#define PBL_KV_RESTART_SAMEPFX 0x02u /* restart word bit 31 (setHasSameKeyPrefix) */
#define PBL_KV_OBSOLETE 0x04u      /* trailer had InternalKeyKindSSTableInternalObsoleteBit */
#define PBL_KV_INVALID_KEY 0x08u   /* key < 8 bytes: kind Invalid, nil user key   */
#define PBL_KV_VALBLK_HANDLE 0x10u /* value bytes are prefix+valblk.Handle        */
#define PBL_KV_BLOB_HANDLE 0x20u   /* value bytes are prefix+blob handle / colblk external */
#define PBL_KV_PREFIX_CHANGED 0x40u /* colblk prefixChanged bit                   */
/* colblk rows: OBSOLETE = isObsolete bit (data_block.go:519); an isValueExternal
   row (data_block.go:1700-1704) is VALBLK_HANDLE or BLOB_HANDLE by its first
   (value-prefix) byte, and its value bytes are the raw column slice; the
   trailer is trailers.At(row) unmasked; entry_off[] is the row index. */

/* ---- batch descriptor ------------------------------------------------------- */
typedef struct pbl_block_batch {
  const uint8_t* blocks;     /* concatenated, already-decompressed block bytes (no 5 B
                                physical trailer).  Must be readable up to the next
                                16-byte boundary after every block.                 */
  const uint64_t* block_off; /* [n_blocks] byte offset of each block in `blocks`    */
  const uint32_t* block_len; /* [n_blocks] byte length of each block (< 4 GiB: the
                                rowblk 64-bit offsets of rowblk_64bit_test.go:28-183
                                are out of scope; blocks are <= 32 KiB in practice
                                and the general path handles any u32 length; a
                                row key past 32768 bytes, which only a longer
                                block can hold, needs the workspace of
                                pbl_workspace_bytes_for)                          */
  uint32_t n_blocks;
  uint32_t format;           /* PBL_FMT_* for every block of the batch              */
  uint32_t flags;            /* PBL_ROW_* flags                                     */
  uint32_t reserved;
  const uint8_t* block_format; /* optional [n_blocks] PBL_FMT_* per block (mixed
                                row + colblk batches); NULL = `format` for all   */
  uint64_t synthetic_seq_num;  /* blockiter.SyntheticSeqNum fused into the decode
                                (transforms.go:90-99; 0 = unset, < 2^56): every
                                decodable key's trailer becomes seq << 8 | kind
                                (rowblk_iter.go:1168-1191, data_block.go:1693-
                                1695); invalid row keys keep the Invalid trailer;
                                ignored with PBL_ROW_RAW_KEYS                    */
} pbl_block_batch;

/* ---- batch totals (device struct, written by the decode kernel) -------------- */
typedef struct pbl_totals {
  uint64_t n_kv;        /* KVs decoded over all blocks                         */
  uint64_t key_bytes;   /* user-key bytes                                      */
  uint64_t val_bytes;   /* value bytes                                         */
  uint64_t n_restarts;  /* restart words (row format)                          */
  uint32_t status_mask; /* OR of (1u << status) over blocks with status != OK  */
  uint32_t n_bad_blocks;/* blocks whose status != PBL_OK                       */
  uint32_t n_slow_blocks;/* blocks decoded by the general (non-LDS) path      */
  uint32_t pad;
} pbl_totals;

/*
 * Output arrays (all caller-allocated, device).  Indexing for block b, KV j:
 *   kv  = blk_kv_base[b] + j                (per-KV arrays)
 *   o   = blk_kv_base[b] + b + j, j<=nkv_b  (per-block N+1 offset arrays)
 * key j of block b  = key_bytes[blk_key_base[b] + key_off[o] .. + key_off[o+1])
 * value j of block b= val_bytes[blk_val_base[b] + val_off[o] .. + val_off[o+1])
 * restart r of b    = restarts[blk_rst_base[b] + r]  (raw LE32 word, bit 31 kept)
 * Optional arrays may be NULL.  The blk_*_base arrays have n_blocks+1 entries; the
 * last entry holds the batch total.  When a capacity is exceeded the kernel still
 * computes every size (totals, blk_*_base) but writes no bytes, and reports
 * PBL_OVERFLOW: re-run with larger buffers.
 */
typedef struct pbl_decode_out {
  uint64_t* trailer;      /* [kv_cap] base.InternalKeyTrailer (obsolete bit cleared) */
  uint8_t* kv_flags;      /* [kv_cap] PBL_KV_* (optional)                        */
  uint32_t* entry_off;    /* [kv_cap] KVEncoding.Offset of each row entry (optional) */
  uint32_t* key_off;      /* [kv_cap + n_blocks] block-relative key offsets       */
  uint32_t* val_off;      /* [kv_cap + n_blocks] block-relative value offsets     */
  uint8_t* key_bytes;     /* [key_cap]                                            */
  uint8_t* val_bytes;     /* [val_cap]                                            */
  uint32_t* restarts;     /* [rst_cap] raw restart words (optional, row format)   */
  uint64_t* blk_kv_base;  /* [n_blocks+1]                                         */
  uint64_t* blk_key_base; /* [n_blocks+1]                                         */
  uint64_t* blk_val_base; /* [n_blocks+1]                                         */
  uint64_t* blk_rst_base; /* [n_blocks+1] (optional)                              */
  uint32_t* blk_status;   /* [n_blocks] PBL_* status per block                    */
  pbl_totals* totals;     /* [1]                                                  */
  uint64_t kv_cap, key_cap, val_cap, rst_cap;
  void* workspace;        /* device scratch of pbl_workspace_bytes(n_blocks) bytes,
                             or of pbl_workspace_bytes_for(n_blocks, longest block);
                             16-byte aligned */
  uint64_t workspace_bytes;
  uint64_t* tiering_span_id; /* [kv_cap] (optional) base.KVMeta.TieringSpanID per KV   */
  uint64_t* tiering_attr;    /* [kv_cap] (optional) base.KVMeta.TieringAttribute per KV;
                                both or neither; see PBL_COL_TIERING                  */
} pbl_decode_out;

/* ABI version of the loaded library (== PBL_ABI_VERSION). */
int pbl_abi_version(void);

/* Device scratch the decode needs for a batch of n_blocks (look-back state). */
uint64_t pbl_workspace_bytes(uint32_t n_blocks);

/*
 * Row keys longer than 32768 bytes (ABI v9).  The general row walk keeps the
 * current key in a 32 KiB LDS buffer; Go's readEntry grows fullKey without
 * bound (rowblk_iter.go:400-403).  With a workspace of pbl_workspace_bytes(n)
 * a row block holding a longer key reports PBL_UNSUPPORTED (every other block
 * of the batch is unaffected).  pbl_workspace_bytes_for lifts the limit: for
 * max_block_len <= 32768 (no block can hold such a key: a key is never longer
 * than its block) it returns pbl_workspace_bytes(n_blocks); otherwise it adds,
 * after the existing layout (whose size and offsets are unchanged; no further
 * id list is needed), PBL_LONGKEY_WGS key spill slots of max_block_len rounded
 * up to 16 bytes each.  Pass the longest block.Handle length of the batch; the
 * lengths are known on the host.  The decode takes the slot size from
 * out->workspace_bytes: (workspace_bytes - pbl_workspace_bytes(n)) /
 * PBL_LONGKEY_WGS rounded down to 16, so a smaller surplus gives smaller slots,
 * and a key that outgrows its slot (more than 32768 - 48 + slot bytes) reports
 * PBL_UNSUPPORTED.  Such blocks are sized and written by PBL_LONGKEY_WGS
 * one-wave workgroups, each looping over the listed blocks with its own slot:
 * a cold path, stream-ordered like the rest; the host reads nothing back.
 */
#ifndef PBL_LONGKEY_WGS
#define PBL_LONGKEY_WGS 32
#endif
uint64_t pbl_workspace_bytes_for(uint32_t n_blocks, uint32_t max_block_len);

/*
 * Decode every block of `batch` into `out` on `stream`: one stream-ordered
 * single-pass launch (plus a memset of the workspace).  Returns PBL_OK or
 * PBL_INVALID_ARG / PBL_DEVICE_ERROR for launch problems; per-block corruption is
 * reported in out->blk_status and out->totals (read them after the stream syncs).
 */
int pbl_decode_batch(const pbl_block_batch* batch, pbl_decode_out* out, void* stream);

/*
 * Size pass: the same parse as pbl_decode_batch, writing only
 * the per-block results: blk_{kv,key,val,rst}_base (n_blocks+1 entries, the last
 * = batch totals), blk_status and totals.  Only those arrays, `totals` and the
 * workspace are required in `out`; every other pointer and capacity is ignored
 * and nothing else is written.  A caller without exact sizes runs this, then
 * pbl_decode_batch into exactly sized buffers (instead of guessing capacities
 * and re-running on PBL_OVERFLOW).  Statuses are those pbl_decode_batch reports,
 * PBL_OVERFLOW excepted.
 */
int pbl_size_batch(const pbl_block_batch* batch, pbl_decode_out* out, void* stream);

/*
 * Layout of the ABI structs as this library was compiled, for binding checks
 * (ctypes, cgo): writes up to `cap` u64 values and returns how many it has:
 *   sizeof(pbl_block_batch), the offsets of its 9 fields in declaration order,
 *   sizeof(pbl_totals), the offsets of its 8 fields,
 *   sizeof(pbl_decode_out), the offsets of its 22 fields,
 *   then likewise pbl_transforms, pbl_footer, pbl_index_out, pbl_kv_out,
 *   pbl_value_out, pbl_kv and pbl_kv_meta (sizeof, then every field's offset in
 *   declaration order).
 */
size_t pbl_struct_layout(uint64_t* out, size_t cap);

/*
 * Offset concat for a sharded batch: add this rank's global
 * bases (exclusive prefix over lower ranks of n_kv / key_bytes / val_bytes /
 * n_restarts, all-gathered over RCCL) to the n_blocks+1 entries of each
 * blk_*_base array.  Per-KV offsets are block-relative and never need rebasing.
 */
int pbl_rebase_blocks(pbl_decode_out* out, uint32_t n_blocks, uint64_t kv_base,
                      uint64_t key_base, uint64_t val_base, uint64_t rst_base,
                      void* stream);


/*
 * Same offset concat, fully stream-ordered: `rank_totals` is the DEVICE array of
 * world*4 u64 {n_kv, key_bytes, val_bytes, n_restarts} per rank exactly as an
 * RCCL all-gather of each rank's pbl_totals prefix leaves it; the kernel forms
 * this rank's exclusive prefix itself (no host round trip).
 */
int pbl_offset_concat(pbl_decode_out* out, uint32_t n_blocks, const uint64_t* rank_totals,
                      uint32_t rank, void* stream);

/* ---- physical blocks: checksums and decompression --------- */
/* Blocks as they sit in an SST: [block bytes][compression indicator u8][checksum
 * LE32] (sstable/block/block.go:539-571); block_len is the block.Handle length
 * (the 5-byte trailer follows it).  The kernels read in aligned 16-B granules:
 * `bytes` must stay readable for 16 bytes past every block's trailer (an SST
 * file's own following bytes, or 16 bytes of padding after the buffer). */
typedef struct pbl_phys_batch {
  const uint8_t* bytes;      /* DEVICE bytes                                           */
  const uint64_t* block_off; /* [n_blocks] DEVICE offset of each block in `bytes`        */
  const uint32_t* block_len; /* [n_blocks] DEVICE block.Handle.Length (trailer excluded) */
  uint32_t n_blocks;
  uint32_t flags;            /* PBL_PHYS_* (0: the defaults)                           */
} pbl_phys_batch;
/* MinLZ blocks in the MinLZ form (first byte 0, internal/compression/minlz.go:
   52-72) are decoded on the device only with this flag: the format is restated
   without bytes from the real encoder to pin it (github.com/minio/minlz is an
   absent dependency), so by default such blocks report
   PBL_UNSUPPORTED and the caller decodes them on the host.  MinLZ blocks in
   the Snappy form (minlz_test.go:31-36) are always decoded.                    */
#define PBL_PHYS_MINLZ_NATIVE 0x1u
enum { /* block.ChecksumType (block.go:106-114) */
  PBL_CHECKSUM_NONE = 0, PBL_CHECKSUM_CRC32C = 1, PBL_CHECKSUM_XXHASH = 2, PBL_CHECKSUM_XXHASH64 = 3
};
enum { /* block.CompressionIndicator (compression.go:170-193) */
  PBL_COMPRESSION_NONE = 0, PBL_COMPRESSION_SNAPPY = 1, PBL_COMPRESSION_ZSTD = 7, PBL_COMPRESSION_MINLZ = 8
};

/*
 * ValidateChecksum (block.go:164-197) for every block: status[b] = PBL_OK or
 * PBL_CORRUPT_CHECKSUM; computed[b] (optional) = the checksum computed over the
 * block bytes and the indicator byte.  CRC32C (internal/crc: Castagnoli, then
 * Value()'s rotation and delta) or XXH64 truncated to 32 bits; other types return
 * PBL_UNSUPPORTED.
 */
int pbl_verify_checksums(const pbl_phys_batch* batch, uint32_t checksum_type, uint32_t* status, uint32_t* computed,
                         void* stream);
/*
 * Decompressor.DecompressedLen (block.go:549-556) of every block: out_len[b];
 * status[b] = PBL_OK, PBL_CORRUPT_COMPRESSION or PBL_UNSUPPORTED (the legacy
 * codecs are not decoded on the device).  Snappy: its uvarint header; zstd: the
 * uvarint Pebble prefixes (zstd_cgo.go:111-119); MinLZ: minlz.DecodedLen
 * (internal/compression/minlz.go:70-73; a block in the Snappy form, first byte
 * not 0, by its Snappy header).
 */
int pbl_decompressed_lengths(const pbl_phys_batch* batch, uint32_t* out_len, uint32_t* status, void* stream);
/*
 * DecompressInto (block.go:557-565): block b's decoded bytes at out + out_off[b]
 * (out_cap[b] bytes available; DEVICE arrays), its length in out_len[b] and
 * status[b] = PBL_OK / PBL_CORRUPT_COMPRESSION / PBL_OVERFLOW / PBL_UNSUPPORTED.
 * Uncompressed blocks are copied; snappy (golang/snappy block format) and zstd
 * (RFC 8878 frames after Pebble's uvarint length, zstd_cgo.go:86-108: the frames
 * must decode to exactly that length; a frame naming a dictionary is
 * PBL_UNSUPPORTED) are decoded on the device.  The outputs form a pbl_block_batch {out,
 * out_off, out_len} for pbl_decode_batch (keep out_off 8-B aligned for colblk).
 * zstd's batch path takes a stream-ordered workspace (hipMallocAsync on `stream`,
 * ~40 KB per block, freed on the stream after its last launch); when that
 * allocation fails every zstd block takes the one-wave-per-block decoder instead.
 */
int pbl_decompress_blocks(const pbl_phys_batch* batch, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                          uint32_t* out_len, uint32_t* status, void* stream);

/* ---- table footer and index blocks ------------------------ */
enum { /* TableFormat (sstable/format.go:20-60); the footer's (magic, version) */
  PBL_TABLE_LEVELDB = 1, PBL_TABLE_ROCKSDBV2 = 2,
  PBL_TABLE_PEBBLEV1 = 3, PBL_TABLE_PEBBLEV2 = 4, PBL_TABLE_PEBBLEV3 = 5, PBL_TABLE_PEBBLEV4 = 6,
  PBL_TABLE_PEBBLEV5 = 7, PBL_TABLE_PEBBLEV6 = 8, PBL_TABLE_PEBBLEV7 = 9, PBL_TABLE_PEBBLEV8 = 10
};
typedef struct pbl_footer {
  uint32_t table_format;   /* PBL_TABLE_*                                               */
  uint32_t checksum_type;  /* PBL_CHECKSUM_* of every block of the table                */
  uint64_t metaindex_off, metaindex_len;
  uint64_t index_off, index_len;  /* the (top-level) index block's handle             */
  uint64_t footer_off, footer_len;
  uint32_t attributes;     /* Pebblev7+ attribute bitset, else 0                        */
  uint32_t reserved;
} pbl_footer;
/*
 * parseFooter (sstable/table.go:328-404) on HOST memory: `buf` holds the last
 * buf_len bytes of a file of file_size bytes (readFooter reads the last
 * maxFooterLen = 61 bytes).  LevelDB, RocksDBv2 and Pebblev1-v8 footers; the
 * Pebblev6+ footer checksum (CRC32C Value) is verified.  Returns PBL_OK or
 * PBL_CORRUPT_FOOTER (bad magic, unsupported version or checksum type, short
 * footer, checksum mismatch, handles past the end of the file).
 */
int pbl_parse_footer(const uint8_t* buf, uint64_t buf_len, uint64_t file_size, pbl_footer* out);

typedef struct pbl_index_out {
  uint64_t* handle_off;  /* [cap] block.Handle.Offset of each entry, in block order              */
  uint64_t* handle_len;  /* [cap] block.Handle.Length                                             */
  uint64_t* props_off;   /* [cap] (nullable) where the entry's block-property bytes start: in the
                            decoded val_bytes (row) or in the batch's block bytes (colblk)         */
  uint32_t* props_len;   /* [cap] (nullable)                                                      */
  uint64_t* blk_base;    /* [n_blocks + 1] first entry of each index block; [n_blocks] = total    */
  uint32_t* blk_status;  /* [n_blocks] PBL_OK / PBL_CORRUPT_INDEX / PBL_CORRUPT_COLBLK_HEADER /
                            PBL_OVERFLOW (or the row decode's status)                             */
  uint64_t cap;          /* entries the handle arrays hold                                         */
} pbl_index_out;
/*
 * rowblk.IndexIter.BlockHandleWithProperties (rowblk/rowblk_index_iter.go:82-84)
 * for every entry of a batch of row-format index blocks that pbl_decode_batch
 * (flags 0) has decoded into `decoded`: entry k's value at
 * val_bytes[blk_val_base[b] + val_off[..]] through block.DecodeHandleWithProperties
 * (block/block.go:80-104: uvarint offset, uvarint length, the rest = properties).
 * Entry k of the handle arrays is KV k of `decoded` (blk_base = blk_kv_base).  A
 * value that is not a handle makes its block PBL_CORRUPT_INDEX.
 */
int pbl_index_handles_row(const pbl_decode_out* decoded, uint32_t n_blocks, pbl_index_out* out, void* stream);
/*
 * colblk.IndexIter over a batch of columnar index blocks (colblk/index_block.go:
 * IndexBlockDecoder.Init :150-156, BlockHandleWithProperties :310-321):
 * separators RawBytes, offsets and lengths Uint, block properties RawBytes;
 * column layout checks as for data blocks (PBL_CORRUPT_COLBLK_HEADER).  Blocks
 * are sized first (blk_base), then written; a total past cap reports
 * PBL_OVERFLOW for the blocks that do not fit and writes none of their entries.
 */
int pbl_index_handles_col(const pbl_block_batch* batch, pbl_index_out* out, void* stream);

typedef struct pbl_kv_out {
  uint64_t* key_off;     /* [cap] where KeyAt(i) starts in the batch's block bytes      */
  uint32_t* key_len;     /* [cap]                                                        */
  uint64_t* val_off;     /* [cap] where ValueAt(i) starts in the batch's block bytes    */
  uint32_t* val_len;     /* [cap]                                                        */
  uint64_t* blk_base;    /* [n_blocks + 1] first entry of each block; [n_blocks] = total */
  uint32_t* blk_status;  /* [n_blocks] PBL_OK / PBL_CORRUPT_COLBLK_HEADER /
                            PBL_CORRUPT_BOUNDS / PBL_OVERFLOW                            */
  uint64_t cap;          /* entries the arrays hold                                       */
} pbl_kv_out;
/*
 * colblk.KeyValueBlockDecoder (colblk/key_value_block.go:76-89) over a batch of
 * key-value blocks -- the metaindex of Pebblev6+ tables and the properties
 * block of Pebblev7+ tables (sstable/reader.go:536-545,601-617;
 * layout.go:789-824): no custom header, column 0 the keys and column 1 the
 * values (RawBytes).  Every row's key and value are reported as slices of the
 * batch's bytes (zero-copy, as KeyAt / ValueAt).  Column layout checks as for
 * data blocks; a slice past its block is PBL_CORRUPT_BOUNDS.  Sized, scanned,
 * then written; a total past cap reports PBL_OVERFLOW for the blocks that do
 * not fit.
 */
int pbl_kv_blocks(const pbl_block_batch* batch, pbl_kv_out* out, void* stream);

/*
 * The value-block index (valblk/valblk.go:338-393) on the device: `vbi` holds
 * the decompressed index block (vbi_len bytes, DEVICE memory), rows of
 * num_w + off_w + len_w little-endian bytes (valblk.IndexHandle widths, each
 * 1..8).  Writes the handle of value block i to handle_off[i] / handle_len[i]
 * for i < min(rows, cap) and *n_blocks = rows (DEVICE u32; rows = vbi_len / row
 * width).  *status (DEVICE u32) = PBL_OK, or PBL_CORRUPT_VALUE_HANDLE when a
 * row's block number is not its index, the block has a partial row, or a
 * width is 0 or > 8 (DecodeIndex's errors).
 */
int pbl_valblk_index(const uint8_t* vbi, uint64_t vbi_len, uint32_t num_w, uint32_t off_w, uint32_t len_w,
                     uint64_t* handle_off, uint64_t* handle_len, uint32_t cap, uint32_t* n_blocks,
                     uint32_t* status, void* stream);

typedef struct pbl_value_out {
  uint32_t* val_off;     /* [kv_cap + n_blocks] block-relative value offsets (as pbl_decode_out) */
  uint8_t* val_bytes;    /* [val_cap]                                                            */
  uint64_t* blk_val_base;/* [n_blocks + 1]; [n_blocks] = total                                   */
  uint32_t* blk_status;  /* [n_blocks] the decode's status, else PBL_OK /
                            PBL_CORRUPT_VALUE_HANDLE / PBL_OVERFLOW                              */
  uint64_t val_cap;
} pbl_value_out;
/*
 * Resolve value-block handles (valueBlockFetcher.Fetch, valblk/reader.go:251-302)
 * for every KV of a decoded batch: a KV whose kv_flags has PBL_KV_VALBLK_HANDLE
 * holds the value prefix byte + valblk.Handle (uvarint ValueLen, BlockNum,
 * OffsetInBlock; valblk.go:218-279); its value becomes
 * value_blocks[BlockNum][OffsetInBlock : OffsetInBlock + ValueLen] of the
 * batch of (decompressed) value blocks.  Every other value is copied as is
 * (blob handles stay handles, as a reader without blob files reports them).
 * `decoded` needs kv_flags, val_off, val_bytes, blk_kv_base, blk_val_base and
 * blk_status.  A handle past its value block, or naming a block past the
 * batch, makes its block PBL_CORRUPT_VALUE_HANDLE.  Sized, scanned, then
 * written; a total past val_cap reports PBL_OVERFLOW for the blocks that do
 * not fit.
 */
int pbl_resolve_values(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_block_batch* value_blocks,
                       pbl_value_out* out, void* stream);

/* ---- blockiter.Transforms on the device ------------------ */
/* Comparer.Split used to find the suffix a SyntheticSuffix replaces. */
enum {
  PBL_SPLIT_WHOLE = 0,    /* base.DefaultSplit: no suffix (internal/base/comparer.go:206-208) */
  PBL_SPLIT_TESTKEYS = 1, /* testkeys.Comparer: before the last '@' (internal/testkeys/testkeys.go:144-150) */
  PBL_SPLIT_CRDB = 2      /* cockroachkvs.Split: last byte = version length (cockroachkvs/cockroachkvs.go:298-309) */
};
typedef struct pbl_transforms {
  uint64_t synthetic_seq_num;    /* blockiter.SyntheticSeqNum; 0 = unset (transforms.go:90-99) */
  uint32_t hide_obsolete_points; /* drop PBL_KV_OBSOLETE KVs (transforms.go:24-27)            */
  uint32_t split;                /* PBL_SPLIT_* (only used with a suffix)                     */
  const uint8_t* prefix;         /* DEVICE bytes of the SyntheticPrefix (transforms.go:120-162) */
  const uint8_t* suffix;         /* DEVICE bytes of the SyntheticSuffix (transforms.go:101-118) */
  uint32_t prefix_len, suffix_len;
  const pbl_block_batch* blocks; /* REQUIRED: the batch `in` was decoded from (host struct,
                                    device arrays).  Row blocks are read by rowblk.Iter
                                    with the prefix inside fullKey (rowblk_iter.go:259-263,
                                    400): a key shorter than 8 B is re-read from its block
                                    and decodes as a valid key when prefix ++ key is 8 B or
                                    longer (:1168-1199), and Split runs on prefix ++ key
                                    (:1183).  Colblk blocks follow their KeySeeker
                                    (data_block.go:444-460; cockroachkvs.go:1073-1089).     */
} pbl_transforms;

/* Device scratch pbl_transform_batch needs in out->workspace. */
uint64_t pbl_transform_workspace_bytes(uint32_t n_blocks);

/*
 * Apply `t` to a decoded batch (`in`, as pbl_decode_batch left it, n_blocks
 * blocks) into `out` (same layout contract; caller-allocated; out->workspace of
 * pbl_transform_workspace_bytes): every visible KV (HideObsoletePoints drops the
 * obsolete ones) keeps its order, flags, entry offset, KVMeta (tiering_span_id /
 * tiering_attr, copied when both `in` and `out` carry them) and value; its trailer
 * takes the synthetic sequence number (InternalKey.SetSeqNum); its user key
 * becomes F[:Split(F)] ++ suffix (suffix set) or F, F = prefix ++ key (row
 * blocks; colblk: prefix ++ key[:Split(key)] ++ suffix); keys of entries that
 * stay PBL_KV_INVALID_KEY are empty and keep the Invalid trailer.  Restart words
 * are the input's; statuses too, except a row block whose transformed iteration
 * would panic (a key made valid by the prefix, kind SET, empty value, value
 * prefix on): PBL_CORRUPT_BOUNDS.  A block whose decode failed stays failed.
 * Keys and values are copied in 16-byte chunks: in->key_bytes, in->val_bytes,
 * t->prefix and t->suffix must be readable 16 bytes past their capacity /
 * length (pebble_amd's allocations pad them).  A workspace memset and three
 * stream-ordered launches (count; scan: tiles of 1024 blocks with decoupled
 * look-back; scatter); on a capacity overflow every decodable block reports
 * PBL_OVERFLOW and only sizes are written.  Replaces the iteration-time transforms of rowblk.Iter
 * (rowblk_iter.go:400,487-517,1168-1187) and colblk.DataBlockIter
 * (data_block.go:1299-1303,1437-1462,1680-1697) for a whole batch.
 */
int pbl_transform_batch(const pbl_decode_out* in, uint32_t n_blocks, const pbl_transforms* t, pbl_decode_out* out,
                        void* stream);

/* ---- rowblk.Writer (format producer; host memory) ---------------------------- */
typedef struct pbl_rowblk_writer pbl_rowblk_writer;
pbl_rowblk_writer* pbl_rowblk_writer_new(int restart_interval);
void pbl_rowblk_writer_free(pbl_rowblk_writer* w);
void pbl_rowblk_writer_reset(pbl_rowblk_writer* w, int restart_interval);
/* rowblk_writer.go:263-286.  `trailer` is base.InternalKeyTrailer. */
int pbl_rowblk_writer_add(pbl_rowblk_writer* w, const uint8_t* user_key, size_t user_key_len,
                          uint64_t trailer, int is_obsolete, const uint8_t* value,
                          size_t value_len, int64_t max_shared_key_len, int add_value_prefix,
                          uint8_t value_prefix, int set_has_same_key_prefix);
/* rowblk_writer.go:323-334 (raw key, no trailer). */
int pbl_rowblk_writer_add_raw(pbl_rowblk_writer* w, const uint8_t* key, size_t key_len,
                              const uint8_t* value, size_t value_len);
size_t pbl_rowblk_writer_estimated_size(const pbl_rowblk_writer* w);
size_t pbl_rowblk_writer_entry_count(const pbl_rowblk_writer* w);
/* Finish; copies the block into `dst` if dst_cap suffices; returns the block size. */
size_t pbl_rowblk_writer_finish(pbl_rowblk_writer* w, uint8_t* dst, size_t dst_cap);

/*
 * Synthetic batch generator (host memory, multithreaded), SURVEY.md §8(d):
 * key of row r = BE64(r) || BE64(splitmix64(seed ^ r)) (key_len 16; longer keys
 * append splitmix bytes), row r = (block << 20) + k, trailer MakeTrailer(r, SET),
 * value bytes from splitmix64(seed + r).  Each block is filled while
 * EstimatedSize()+entry <= block_size and is placed at a fixed `block_size`
 * stride in `dst` (dst must hold n_blocks*block_size bytes).  Fills
 * block_off/block_len (host arrays) and returns total KVs.  Block content
 * depends only on (seed, global block index).
 */
uint64_t pbl_gen_row_blocks(uint64_t seed, uint32_t n_blocks, uint32_t block_size,
                            int restart_interval, uint32_t key_len, uint32_t val_len,
                            int value_prefix, uint8_t* dst, uint64_t* block_off,
                            uint32_t* block_len, int n_threads);
/* The same from global block `first_block` on (output block i = global block
 * first_block + i: a rank's shard of one global batch), with obsolete points
 * (HideObsoletePoints measurements): key k of a block carries the trailer's
 * obsolete bit when obsolete_every > 0 and k % obsolete_every ==
 * obsolete_every - 1 (rowblk_writer.go:30-42).                              */
uint64_t pbl_gen_row_blocks_obs(uint64_t seed, uint32_t first_block, uint32_t n_blocks, uint32_t block_size,
                                int restart_interval, uint32_t key_len, uint32_t val_len,
                                int value_prefix, uint32_t obsolete_every, uint8_t* dst,
                                uint64_t* block_off, uint32_t* block_len, int n_threads);

/* ---- colblk.DataBlockEncoder (format producer; host memory) ------------------ */
/*
 * sstable/colblk/data_block.go:600-790 with colblk.DefaultKeySchema
 * (schema PBL_FMT_COL_DEFAULT, key prefix = bytes before the first '@', the
 * testkeys comparer; data_block.go:207-345) or cockroachkvs.KeySchema
 * (PBL_FMT_COL_CRDB1, cockroachkvs/cockroachkvs.go:505-766).
 */
typedef struct pbl_colblk_writer pbl_colblk_writer;
pbl_colblk_writer* pbl_colblk_writer_new(uint32_t schema, int bundle_size);
void pbl_colblk_writer_free(pbl_colblk_writer* w);
void pbl_colblk_writer_reset(pbl_colblk_writer* w);
/* Add one KV (DataBlockEncoder.Add after KeyWriter.ComparePrev).  prefix_len < 0
 * = the schema's Split.  value_kind: 0 in place, 1 valblk handle, 2 blob handle
 * (stored as prefix byte || value, isValueExternal set).  Returns 1 when the key's
 * prefix equals the previous key's, 0 otherwise, PBL_INVALID_ARG (7) on a bad key. */
int pbl_colblk_writer_add(pbl_colblk_writer* w, const uint8_t* key, size_t key_len, int64_t prefix_len,
                          uint64_t trailer, const uint8_t* value, size_t value_len, int value_kind,
                          int is_obsolete);
/* Pebblev8 data blocks (sstable/format.go:305-316): DataBlockEncoder.Init with
 * WithTieringColumns() (data_block.go:610-627).  Call on a fresh or reset writer,
 * before the first add; the setting survives pbl_colblk_writer_reset. */
void pbl_colblk_writer_set_tiering(pbl_colblk_writer* w, int tiering);
/* DataBlockEncoder.AddWithSecondaryBlobHandle (data_block.go:712-765) with a
 * base.KVMeta: the meta is stored only when its attribute is non-zero
 * (KVMeta.IsSet, internal/base/internal.go:698-702), and meta and handle are
 * ignored unless the writer has the tiering columns.  Same returns as
 * pbl_colblk_writer_add. */
int pbl_colblk_writer_add_meta(pbl_colblk_writer* w, const uint8_t* key, size_t key_len, int64_t prefix_len,
                               uint64_t trailer, const uint8_t* value, size_t value_len, int value_kind,
                               int is_obsolete, uint64_t tiering_span_id, uint64_t tiering_attr,
                               const uint8_t* secondary_handle, size_t secondary_handle_len);
uint32_t pbl_colblk_writer_rows(const pbl_colblk_writer* w);
/* DataBlockEncoder.Size() as it was at `rows` rows (rows() or rows()-1). */
size_t pbl_colblk_writer_size(const pbl_colblk_writer* w, uint32_t rows);
/* Finish(rows, Size(rows)) with rows == rows() or rows()-1; copies the block to
 * dst when dst_cap suffices; returns the block size (0 on a bad row count).  The
 * writer must be reset before reuse. */
size_t pbl_colblk_writer_finish(pbl_colblk_writer* w, uint32_t rows, uint8_t* dst, size_t dst_cap);

/* cockroachkvs.KeyGenConfig (cockroachkvs/test_utils.go) + value length. */
typedef struct pbl_colgen_config {
  uint64_t seed;
  uint32_t alphabet_len;       /* PrefixAlphabetLen                        */
  uint32_t prefix_len_shared;  /* PrefixLenShared                          */
  uint32_t roach_key_len;      /* RoachKeyLen                              */
  uint32_t avg_keys_per_prefix;/* AvgKeysPerPrefix                         */
  uint64_t base_wall_time;     /* BaseWallTime                             */
  uint32_t pct_logical;        /* PercentLogical                           */
  uint32_t value_len;
  uint32_t obsolete_every;     /* 0, or: row k of a block has isObsolete set
                                  when k % obsolete_every == obsolete_every-1
                                  (HideObsoletePoints measurements)         */
  uint32_t tiering;            /* 0, or: Pebblev8 blocks with the tiering
                                  columns; row k's KVMeta is span 1 + r % tiering,
                                  attribute (base_wall_time / 1e9) + r % 3600,
                                  unset (KVMeta{}) for one row in ten, r drawn
                                  per row from the block's seed             */
  uint32_t first_block;        /* global index of the first block generated:
                                  block i of the output is global block
                                  first_block + i (a rank's shard of one
                                  global batch)                              */
  uint32_t reserved;
} pbl_colgen_config;

/*
 * Synthetic colblk batch (config 3): per block, sorted KVs drawn per
 * cockroachkvs.RandomKVs with a per-block seed, trailer MakeTrailer((block<<20)+k,
 * SET), random value bytes; rows are added while the finished block stays
 * <= block_size (Finish(rows-1) on overflow, as the sstable writer does) and
 * blocks are placed at a fixed `block_size` stride.  Returns total rows.
 */
uint64_t pbl_gen_col_blocks(const pbl_colgen_config* cfg, uint32_t schema, uint32_t n_blocks,
                            uint32_t block_size, uint8_t* dst, uint64_t* block_off,
                            uint32_t* block_len, int n_threads);

/* Config 5 (BASELINE.json configs[4]): Zipf(s)-skewed key and value lengths. */
typedef struct pbl_zipf_config {
  uint64_t seed;
  uint32_t key_min, key_max;   /* user-key length range, key_min >= 8 (8, 1024)  */
  uint32_t val_min, val_max;   /* value length range (0, 65536)                   */
  double s;                    /* Zipf exponent (1.1)                             */
  uint32_t block_size;         /* target block size; a block always takes its
                                  first KV, so one large KV may exceed it         */
  int32_t restart_interval;    /* row format only (1, 16, 32)                     */
  uint32_t first_block;        /* output block i = global block first_block + i   */
  uint32_t reserved;
} pbl_zipf_config;

/*
 * Synthetic config-5 batch in host memory: format PBL_FMT_ROW (rowblk.Writer)
 * or PBL_FMT_COL_DEFAULT (DataBlockEncoder + DefaultKeySchema).  Key of row k of
 * block b: 8 base-26 letters of (b << 20) + k, then random letters to its Zipf
 * length; trailer MakeTrailer((b << 20) + k, SET); random value bytes.  Blocks
 * are variable-length, packed at 8-B alignment into dst; *bytes_used is the
 * packed size.  Returns total KVs, or UINT64_MAX on a bad config or when
 * dst_cap < *bytes_used (nothing copied).
 */
uint64_t pbl_gen_zipf_blocks(const pbl_zipf_config* cfg, uint32_t format, uint32_t n_blocks,
                             uint8_t* dst, uint64_t dst_cap, uint64_t* block_off, uint32_t* block_len,
                             uint64_t* bytes_used, int n_threads);

/* ---- blockiter.Data over one decoded block (host side) ----
 * The adapter a Go shim exposes behind sstable/blockiter
 * (sstable/blockiter/block_iter.go:19-108): rowblk.Iter / colblk.DataBlockIter
 * positioning over the arrays of a decoded batch COPIED TO HOST MEMORY (every
 * pointer of `host` is a host pointer; nothing here touches the device).  A
 * positioning call returns the KV it lands on or NULL (exhausted); the pbl_kv
 * it points to lives in the iterator and is valid until the next call. */
#define PBL_CMP_DEFAULT 0u  /* base.DefaultComparer: bytes.Compare, Split = len   */
#define PBL_CMP_TESTKEYS 1u /* testkeys.Comparer (internal/testkeys/testkeys.go)  */
#define PBL_CMP_CRDB 2u     /* cockroachkvs.Comparer (cockroachkvs/cockroachkvs.go) */

typedef struct pbl_kv {   /* base.InternalKV over the decoded arrays (block/kv.go) */
  const uint8_t* user_key;
  uint64_t user_key_len;
  uint64_t trailer;       /* InternalKeyTrailer, as decoded (transforms applied) */
  const uint8_t* value;   /* in-place value bytes, or the handle bytes          */
  uint64_t value_len;
  uint32_t kv_flags;      /* PBL_KV_*                                          */
  uint32_t reserved;
} pbl_kv;

typedef struct pbl_kv_meta { /* base.KVMeta (internal/base/internal.go:686-689)    */
  uint64_t tiering_span_id;
  uint64_t tiering_attribute;
} pbl_kv_meta;

typedef struct pbl_data_iter pbl_data_iter;
pbl_data_iter* pbl_data_iter_new(void);
void pbl_data_iter_free(pbl_data_iter* it);
/* InitHandle (block_iter.go:84-90) for block `block` of a decoded batch of
 * n_blocks: PBL_OK, or the block's decode status (the iterator is then
 * invalidated), or PBL_INVALID_ARG.  hide_obsolete_points: the
 * HideObsoletePoints transform (KVs with PBL_KV_OBSOLETE are skipped). */
int pbl_data_iter_init(pbl_data_iter* it, const pbl_decode_out* host, uint32_t n_blocks, uint32_t block,
                       uint32_t comparer, uint32_t hide_obsolete_points);
const pbl_kv* pbl_data_iter_first(pbl_data_iter* it);
const pbl_kv* pbl_data_iter_last(pbl_data_iter* it);
const pbl_kv* pbl_data_iter_next(pbl_data_iter* it);
const pbl_kv* pbl_data_iter_prev(pbl_data_iter* it);
const pbl_kv* pbl_data_iter_seek_ge(pbl_data_iter* it, const uint8_t* key, uint64_t key_len, uint32_t flags);
const pbl_kv* pbl_data_iter_seek_lt(pbl_data_iter* it, const uint8_t* key, uint64_t key_len, uint32_t flags);
/* FirstWithMeta / NextWithMeta / SeekGEWithMeta (colblk data_block.go:1574-1600;
 * the MetaIterator of sstable/reader_iter.go:26-33): the same positioning, and
 * *meta = the KV's KVMeta from the decoded tiering_span_id / tiering_attr
 * arrays, or KVMeta{} when the iterator lands on no KV or the arrays were not
 * decoded (NULL in `host`, as for row blocks and non-tiering formats). */
const pbl_kv* pbl_data_iter_first_with_meta(pbl_data_iter* it, pbl_kv_meta* meta);
const pbl_kv* pbl_data_iter_next_with_meta(pbl_data_iter* it, pbl_kv_meta* meta);
const pbl_kv* pbl_data_iter_seek_ge_with_meta(pbl_data_iter* it, const uint8_t* key, uint64_t key_len,
                                              uint32_t flags, pbl_kv_meta* meta);
/* (kv, 0) same prefix; (NULL, 1) positioned at a KV of another prefix; (NULL, 0) none */
const pbl_kv* pbl_data_iter_seek_prefix_ge(pbl_data_iter* it, const uint8_t* key, uint64_t key_len, uint32_t flags,
                                           int* prefix_did_not_match);
const pbl_kv* pbl_data_iter_next_with_same_prefix(pbl_data_iter* it, int* prefix_exhausted);
const pbl_kv* pbl_data_iter_next_prefix(pbl_data_iter* it, const uint8_t* succ_key, uint64_t succ_len);
int pbl_data_iter_is_lower_bound(const pbl_data_iter* it, const uint8_t* key, uint64_t key_len);
int pbl_data_iter_valid(const pbl_data_iter* it);
const pbl_kv* pbl_data_iter_kv(pbl_data_iter* it);
void pbl_data_iter_invalidate(pbl_data_iter* it);
int pbl_data_iter_is_data_invalidated(const pbl_data_iter* it);
/* the comparers themselves (Compare < 0 / 0 / > 0, Split) */
int pbl_key_compare(uint32_t comparer, const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len);
uint64_t pbl_key_split(uint32_t comparer, const uint8_t* key, uint64_t key_len);

/* ---- batched SeekGE / SeekLT over a decoded batch, on the device ----
 * Many keys positioned in one stream-ordered launch over the arrays a decode
 * left in device memory: no copy to the host, no per-key call.  The semantics
 * are the host iterator's above (same comparers, same HideObsoletePoints skip).
 *
 * `decoded` is a HOST struct of DEVICE arrays exactly as pbl_decode_batch left
 * it (or pbl_transform_batch, or pbl_resolve_values: the convention of
 * pbl_transform_batch's `in`).  blk_status, blk_kv_base, blk_key_base, key_off
 * and key_bytes are needed; kv_flags only with hide_obsolete_points.  key_bytes
 * and the queries' key_bytes must be readable 16 B past their end (keys are
 * compared 16 B at a time; pebble_amd's allocations pad).
 *
 * Per-block mode (q->block != NULL): blockiter.Data.SeekGE / SeekLT
 * (sstable/blockiter/block_iter.go:19-108; rowblk_iter.go:606-781, :782-1054)
 * in block q->block[i]: the result equals pbl_data_iter_init(block, comparer,
 * hide) followed by pbl_data_iter_seek_ge / _seek_lt.  out.kv = the landing
 * KV's index blk_kv_base[b] + j, or PBL_SEEK_NONE where the iterator returns
 * NULL.  A block id >= n_blocks, or a block whose status is not PBL_OK, gives
 * PBL_SEEK_NONE with PBL_SEEK_BAD_BLOCK (the entry points are asynchronous: it
 * cannot be a return code).  Needs no workspace (NULL, 0).
 *
 * Table mode (q->block == NULL): singleLevelIterator.SeekGE / SeekLT
 * (sstable/reader_iter_single_lvl.go:757-898: index.SeekGE, data.SeekGE, then
 * on into the next block when this one is exhausted).  SeekGE: the first
 * visible KV, in batch order, whose user key is >= the query; SeekLT: the last
 * visible KV whose user key is < the query; PBL_SEEK_NONE past either end.
 * Blocks whose status is not PBL_OK are passed over: a corrupt block publishes
 * zero KVs, key bytes and value bytes (its look-back aggregate is zero in every
 * decode kernel, e.g. rowblk_pool.hip.h block_describe), so it owns no KV index;
 * a block that reports PBL_OVERFLOW keeps its index range but nothing of it was
 * written, and it is passed over by its status like the others.  With
 * hide_obsolete_points the skip over hidden KVs crosses any number of block
 * boundaries.  Precondition: user keys are non-decreasing under `comparer` over
 * the whole batch, as a table's data blocks are.  For an unordered batch the
 * result is unspecified, but every read stays in bounds and the kernel
 * terminates.
 *
 * pbl_seek_prepare builds what table mode needs in `workspace` (DEVICE,
 * 16-byte aligned, pbl_seek_workspace_bytes(n_blocks)): the fence table, one
 * 32-byte record per PBL_OK block that holds a KV, in batch order -- the first
 * 16 bytes of the block's last user key's Split-prefix, so that most steps of
 * the search over blocks are decided without touching key_bytes.  Two
 * launches, no host read.  The workspace is read-only afterwards: any number of
 * pbl_seek_batch calls, on any stream ordered after the prepare, reuse it.  It
 * is bound to one comparer and one batch, and using it with q->comparer equal to
 * prepare's is the caller's precondition: the host keeps no state and reads no
 * device memory, so this cannot be a return code.  The kernel checks it
 * instead: the comparer and n_blocks are recorded in the workspace header, and
 * a table-mode launch that finds another comparer, another n_blocks or no
 * header answers every query PBL_SEEK_NONE with PBL_SEEK_BAD_BLOCK.
 *
 * PBL_INVALID_ARG, before any device call: comparer > PBL_CMP_CRDB, op >
 * PBL_SEEK_LT, NULL decoded / q / out, NULL out->kv, NULL q->key_off, a needed
 * array of `decoded` NULL, a workspace that is not 16-byte aligned or shorter
 * than pbl_seek_workspace_bytes(n_blocks), table mode without a workspace.
 * n == 0 returns PBL_OK without a launch.
 */
#define PBL_SEEK_GE 0u
#define PBL_SEEK_LT 1u
#define PBL_SEEK_NONE UINT64_MAX      /* out.kv: no KV (exhausted) */
#define PBL_SEEK_EXACT       0x1u     /* landing KV's user key compares equal to the query (GE only) */
#define PBL_SEEK_SAME_PREFIX 0x2u     /* landing KV's Split-prefix equals the query's (what SeekPrefixGE
                                         tests, rowblk_iter.go:550-564) */
#define PBL_SEEK_BAD_BLOCK   0x4u     /* per-block mode: the named block is past n_blocks or its status !=
                                         PBL_OK; table mode: the workspace is not this batch's and comparer's */

typedef struct pbl_seek_queries {
  const uint8_t*  key_bytes;  /* DEVICE; readable 16 B past the last key */
  const uint64_t* key_off;    /* DEVICE [n + 1] */
  const uint32_t* block;      /* DEVICE [n], or NULL (see modes) */
  uint32_t n, comparer /* PBL_CMP_* */, op /* PBL_SEEK_* */, hide_obsolete_points;
} pbl_seek_queries;

typedef struct pbl_seek_out {
  uint64_t* kv;     /* DEVICE [n] global KV index (blk_kv_base[b] + j) or PBL_SEEK_NONE */
  uint32_t* block;  /* DEVICE [n], optional: block of the landing KV (0 with PBL_SEEK_NONE) */
  uint8_t*  flags;  /* DEVICE [n], optional: PBL_SEEK_* flag bits */
} pbl_seek_out;

uint64_t pbl_seek_workspace_bytes(uint32_t n_blocks);
int pbl_seek_prepare(const pbl_decode_out* decoded, uint32_t n_blocks, uint32_t comparer,
                     void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_seek_batch(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_seek_queries* q,
                   pbl_seek_out* out, const void* workspace, uint64_t workspace_bytes, void* stream);
/* The same search (one function, seek_core.hip.h seek_one) over arrays in HOST memory
 * (DecodedBatch.to_host(), the oracle's arrays): every pointer of `host`, `q`
 * and `out` is a host pointer; no device call; nothing is read past a key's
 * end.  Table mode builds its fence per call.  Single-threaded. */
int pbl_seek_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q,
                        pbl_seek_out* out);
/* Layout of the two structs above, as pbl_struct_layout reports the others
 * (whose list is unchanged): sizeof(pbl_seek_queries), its 7 field offsets,
 * sizeof(pbl_seek_out), its 3 field offsets. */
size_t pbl_seek_struct_layout(uint64_t* out, size_t cap);

/* ---- batched bounded scans over a decoded batch, on the device ----
 * Query i with bounds [lower_i, upper_i) receives exactly the KVs that a
 * singleLevelIterator over the batch returns for SetBounds(lower, upper);
 * First(); Next()... (sstable/reader_iter_single_lvl.go:443-473, :1367-1390,
 * :1573-1647, skipForward :1765-1840), compacted and copied inside HBM.  The
 * comparers are those of the seeks above (key_cmp.hip.h) and `decoded` is as
 * pbl_seek_batch takes it; trailer, val_off, val_bytes and blk_val_base are
 * needed too, and key_bytes / val_bytes must be readable 16 B past their end.
 *
 * Table mode (q->block == NULL): blocks in batch order, from the landing of
 * SeekGE(lower) to the last KV before the first whose user key is >= upper.  A
 * block whose status is not PBL_OK is passed over (a PBL_OVERFLOW block, which
 * keeps a KV range, included).  With hide_obsolete_points the KVs carrying
 * PBL_KV_OBSOLETE are skipped wherever they lie.  Per-block mode (q->block
 * given): the same scan confined to block q->block[i]; a block id >= n_blocks
 * gives an empty result with status PBL_INVALID_ARG, a block that is not
 * PBL_OK an empty result with that block's status.  An empty lower bound is
 * First().  "No upper bound" is the per-query flag PBL_SCAN_NO_UPPER (q->flags),
 * not an empty key; upper <= lower gives an empty result.  The upper bound is
 * always exclusive: endKeyInclusive belongs to virtual tables and is out of
 * scope, and so is a per-query limit on the number of KVs.  Queries are
 * independent: overlapping queries each receive a full copy.
 *
 * The result has the layout of a decoded batch with one "block" per query:
 * out->result is filled so that kv = blk_kv_base[q] + j, offsets at
 * blk_kv_base[q] + q + j (n_q + 1 of them), key_off / val_off relative to the
 * query's first byte, blk_status[q], totals (n_bad_blocks = queries whose
 * status is not PBL_OK).  `restarts` is unused (n_restarts = 0), blk_rst_base
 * is zeros when given, entry_off and the two tiering arrays are copied when
 * both sides have them, kv_flags when the result has it.  Everything that
 * reads a decoded batch reads a scan result: pbl_data_iter_init(result, n, q,
 * ...), per-block pbl_seek_batch, pbl_scan_batch again.  A query whose key or
 * value bytes would pass 4 GiB reports PBL_UNSUPPORTED and an empty result (the
 * offsets are u32).  Optional: range[2q], range[2q + 1] = the source KV index
 * range [kv_lo, kv_hi) of the query before anything is hidden or passed over
 * (kv_lo == kv_hi for an empty one); src_kv[k] = the source KV index of result
 * KV k.
 *
 * pbl_scan_prepare (depends on the batch, the comparer and the hide flag only)
 * builds in the workspace the seek fence of pbl_seek_prepare and the visible
 * prefix: per aligned tile of 256 source KVs, the exclusive prefix of {visible
 * KVs, their key bytes, their value bytes} and the tile's first block (28 B per
 * 256 KVs); visible = block PBL_OK and not (hide and obsolete).  `n_kv` is the
 * batch's totals.n_kv as the host read it (the workspace is sized by it).
 * pbl_scan_size then writes blk_*_base, blk_status and totals of out->result
 * and out->range only (no other array or capacity of out->result is read);
 * pbl_scan_batch does everything.  When a capacity (kv_cap, key_cap, val_cap)
 * is exceeded, pbl_scan_batch writes every size and no bytes, and reports
 * PBL_OVERFLOW in totals.status_mask.  With PBL_SCAN_SIZED in `flags`,
 * pbl_scan_batch takes the bounds from the workspace as the last pbl_scan_size
 * with the same queries left them, and runs no search.  All launches are
 * stream-ordered; no host synchronisation, no global state.  The workspace
 * (DEVICE, 16-byte aligned, pbl_scan_workspace_bytes(n_queries, n_blocks,
 * n_kv): nothing in it scales with the ranges' lengths) serves one size / batch
 * call at a time; the part prepare wrote is only read by them, so any number
 * of calls with at most n_queries queries, ordered after the prepare, reuse it.
 * A workspace whose header names another comparer (table mode), n_blocks, hide
 * flag or a smaller n_kv than the batch holds gives every query an empty
 * result with status PBL_INVALID_ARG.
 *
 * PBL_INVALID_ARG, before any device call: NULL decoded / q / out or a needed
 * array, comparer > PBL_CMP_CRDB, hide_obsolete_points without kv_flags, only
 * one of the tiering arrays, a workspace that is NULL, not 16-byte aligned or
 * shorter than pbl_scan_workspace_bytes(q->n, n_blocks, n_kv), unknown flags.
 */
#define PBL_SCAN_NO_UPPER 0x1u  /* pbl_scan_queries.flags[i]: no upper bound (upper key i is ignored) */
#define PBL_SCAN_SIZED    0x1u  /* pbl_scan_batch flags: bounds are in the workspace (see above) */

typedef struct pbl_scan_queries {
  const uint8_t*  lower_bytes; /* DEVICE; readable 16 B past the last key */
  const uint64_t* lower_off;   /* DEVICE [n + 1] */
  const uint8_t*  upper_bytes; /* DEVICE; readable 16 B past the last key */
  const uint64_t* upper_off;   /* DEVICE [n + 1] */
  const uint8_t*  flags;       /* DEVICE [n] PBL_SCAN_* per query, or NULL (all 0) */
  const uint32_t* block;       /* DEVICE [n], or NULL (see modes) */
  uint32_t n, comparer /* PBL_CMP_* */, hide_obsolete_points, reserved;
} pbl_scan_queries;

typedef struct pbl_scan_out {
  pbl_decode_out result;  /* one "block" per query (see above); workspace fields unused */
  uint64_t* range;        /* DEVICE [2n], optional */
  uint64_t* src_kv;       /* DEVICE [result.kv_cap], optional */
} pbl_scan_out;

uint64_t pbl_scan_workspace_bytes(uint32_t n_queries, uint32_t n_blocks, uint64_t n_kv);
int pbl_scan_prepare(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, uint32_t comparer,
                     uint32_t hide_obsolete_points, void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_scan_size(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, const pbl_scan_queries* q,
                  pbl_scan_out* out, void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_scan_batch(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, const pbl_scan_queries* q,
                   pbl_scan_out* out, void* workspace, uint64_t workspace_bytes, uint32_t flags, void* stream);
/* The same bounds search (one function, scan.hip bounds_one over seek_core.hip.h)
 * over arrays in HOST memory, followed by a plain gather: every pointer is a
 * host pointer, no device call, no workspace, nothing read past a key's end.
 * Sizes, statuses, overflow rule and outputs as pbl_scan_batch.  Single-threaded. */
int pbl_scan_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_scan_queries* q, pbl_scan_out* out);
/* sizeof(pbl_scan_queries), its 10 field offsets, sizeof(pbl_scan_out), its 3
 * field offsets (pbl_struct_layout's and pbl_seek_struct_layout's lists are unchanged). */
size_t pbl_scan_struct_layout(uint64_t* out, size_t cap);

/* ---- batched k-way merge of sorted decoded batches, on the device ----
 * n_runs decoded batches ("runs", 1 <= n_runs <= PBL_MERGE_MAX_RUNS), all with
 * the same n_blocks, go in; one decoded batch comes out.  Result block q is the
 * merge of block q of every run: exactly the sequence mergingIter.First();
 * Next()... yields over those inputs.  The usual runs are scan results of
 * several tables for the same ranges (one "block" per range), and every run is
 * as pbl_scan_batch takes a batch (key_bytes / val_bytes readable 16 B past
 * their end).
 *
 * Order: mergingIterHeap.less / base.InternalCompare (merging_iter_heap.go:55-67,
 * internal/base/internal.go:431-437): user key ascending under the comparer
 * (PBL_CMP_DEFAULT / TESTKEYS / CRDB, key_cmp.hip.h), then trailer DESCENDING.
 * Ties: two KVs that compare equal in both go in run order, the lower run index
 * first; within a run they keep the run's order.  (The reference leaves that
 * case to the shape of its heap, and it does not arise between the levels of
 * one LSM, whose sequence numbers are distinct.)
 *
 * Out of scope: nothing is dropped or collapsed.  Shadowed versions,
 * tombstones, snapshots, MERGE operands, range deletions and compact.Iter are
 * the consumer's; hiding obsolete points is the scan's job (pbl_scan_batch)
 * and is not repeated here.
 *
 * The result has the layout of a decoded batch with one block per q, as a scan
 * result: kv = blk_kv_base[q] + j, offsets at blk_kv_base[q] + q + j (n_q + 1
 * of them), key_off / val_off relative to the block's first byte,
 * blk_status[q], totals (n_bad_blocks = result blocks whose status is not
 * PBL_OK).  `restarts` is unused (n_restarts = 0), blk_rst_base is zeros when
 * given.  kv_flags, entry_off and the two tiering arrays are copied when the
 * result has them; a run without one of them gives zeros there.  Optional:
 * src_run[k] = the run result KV k came from, src_kv[k] = its KV index in
 * that run.  Everything that reads a decoded batch reads a merge result,
 * pbl_merge_batch included.
 *
 * A result block is empty, and its neighbours are unaffected, when
 *  - a run's block q is not PBL_OK: the result block gets the first non-OK
 *    status among block q of the runs, in run order;
 *  - the summed KV count reaches 2^32, or the summed key or value bytes pass
 *    4 GiB (the offsets are u32): PBL_UNSUPPORTED;
 *  - a run's block q is not sorted under (comparer, trailer descending),
 *    non-strictly, so that a merge result can be merged again:
 *    PBL_INVALID_ARG.  An unsorted input never leads to a read or write
 *    outside the arrays.
 *
 * pbl_merge_size writes blk_*_base, blk_status and totals of out->result only
 * (no other array or capacity of out->result is read); pbl_merge_batch does
 * everything.  When a capacity (kv_cap, key_cap, val_cap) is exceeded,
 * pbl_merge_batch writes every size and no bytes, and reports PBL_OVERFLOW in
 * totals.status_mask.  With PBL_MERGE_SIZED in `flags`, pbl_merge_batch takes
 * the statuses and sizes from the workspace as the last pbl_merge_size over the
 * same runs left them and does not validate again.  All launches are
 * stream-ordered; no host synchronisation, no global state.  The workspace
 * (DEVICE, 16-byte aligned, pbl_merge_workspace_bytes(n_runs, n_blocks,
 * n_kv_total), known before any data is read) serves one call at a time;
 * n_kv_total is the sum of the runs' totals.n_kv as the host read them.  Runs
 * that hold more KVs than that give every block PBL_INVALID_ARG.
 *
 * PBL_INVALID_ARG, before any device call: NULL runs / out or a needed array,
 * n_runs of 0 or more than PBL_MERGE_MAX_RUNS, comparer > PBL_CMP_CRDB, only
 * one of the tiering arrays (in a run or in the result), a workspace that is
 * NULL, not 16-byte aligned or too short, unknown flags.
 */
#define PBL_MERGE_MAX_RUNS 16
#define PBL_MERGE_SIZED 0x1u  /* pbl_merge_batch flags: statuses and sizes are in the workspace (see above) */

typedef struct pbl_merge_runs {
  const pbl_decode_out* runs; /* HOST array [n_runs]; the arrays each names are DEVICE (HOST for
                                 pbl_merge_batch_host); capacities and workspace fields unused */
  uint32_t n_runs, n_blocks, comparer /* PBL_CMP_* */, reserved;
  uint64_t n_kv_total;        /* see above; unused by pbl_merge_batch_host */
} pbl_merge_runs;

typedef struct pbl_merge_out {
  pbl_decode_out result;  /* one block per q (see above); workspace fields unused */
  uint8_t* src_run;       /* [result.kv_cap], optional */
  uint64_t* src_kv;       /* [result.kv_cap], optional */
} pbl_merge_out;

uint64_t pbl_merge_workspace_bytes(uint32_t n_runs, uint32_t n_blocks, uint64_t n_kv_total);
int pbl_merge_size(const pbl_merge_runs* runs, pbl_merge_out* out, void* workspace, uint64_t workspace_bytes,
                   void* stream);
int pbl_merge_batch(const pbl_merge_runs* runs, pbl_merge_out* out, void* workspace, uint64_t workspace_bytes,
                    uint32_t flags, void* stream);
/* The same order (one function, key_cmp.hip.h ikey_cmp) over arrays in HOST
 * memory by a different algorithm: a plain k-way merge that repeatedly takes
 * the least head, the lowest run among equals, so that the two check each
 * other.  No device call, no workspace, nothing read past a key's end.  Sizes,
 * statuses, overflow rule and outputs as pbl_merge_batch.  Single-threaded. */
int pbl_merge_batch_host(const pbl_merge_runs* runs, pbl_merge_out* out);
/* sizeof(pbl_merge_runs), its 6 field offsets, sizeof(pbl_merge_out), its 3
 * field offsets (the other layout lists are unchanged). */
size_t pbl_merge_struct_layout(uint64_t* out, size_t cap);

/* ---- batched snapshot-visible view of a sorted decoded batch, on the device ----
 * One decoded batch goes in, one comes out with the same n_blocks.  Every input
 * block is sorted under (comparer, trailer descending), as a merge result, a
 * scan result or a decode of one table's blocks is.  Result block q is what
 * Iterator.First(); Next()... returns over block q's KVs as the point-key
 * stream, with DefaultMerger: the step pebble.Iterator.findNextEntry /
 * mergeNext takes on top of mergingIter.  Blocks are independent: a user key
 * that ends block q and starts block q + 1 gives two groups.
 *
 * Per block:
 *  1. Visibility (base.Visible, internal/base/internal.go:524; the filter sits
 *     in mergingIter, merging_iter.go:766): a KV is visible iff
 *     trailer >> 8 < snapshot.  A snapshot of PBL_SEQNUM_MAX (or more) sees
 *     everything, sequence number PBL_SEQNUM_MAX included.  The batch bit
 *     (base.SeqNumBatchBit) is NOT interpreted: an indexed batch's keys are
 *     not special here.  Invisible KVs are skipped everywhere, inside a MERGE
 *     chain too.
 *  2. A group is a maximal sequence of KVs whose user keys compare equal under
 *     the comparer (the reference's i.equal).  Under TESTKEYS and CRDB keys
 *     with different bytes can be equal; a result carries the bytes of the KV
 *     that produced it.
 *  3. The head is the group's first visible KV (iterator.go:649-664):
 *     DEL / SINGLEDEL / DELSIZED: the group yields nothing.
 *     SET / SETWITHDEL: one result KV.  Key, trailer, value, tiering meta,
 *     entry_off and the value-kind flag bits (PBL_KV_VALBLK_HANDLE /
 *     PBL_KV_BLOB_HANDLE) are the head's; the other flag bits are zero.
 *     MERGE (iterator.go:1239-1305): the following visible KVs of the group are
 *     gone through.  A MERGE is an operand and continues the chain; a SET /
 *     SETWITHDEL is an operand and ends it; a deletion kind ends it without
 *     being an operand; so does the group's end.  One result KV: key, trailer
 *     and the rest are the head's, the value is the operands' values
 *     concatenated OLDEST FIRST (AppendValueMerger with MergeOlder prepending,
 *     internal/base/merger.go).
 *  4. With PBL_VISIBLE_KEEP_OPERANDS every operand of a chain is a result KV of
 *     its own, in source order (newest first), unconcatenated, for a caller
 *     with its own merger.  Groups headed by a SET are as above.
 *  5. Statuses.  A result block is empty, its neighbours unaffected, when
 *      - the input block is not PBL_OK: that status;
 *      - the block is not sorted under (comparer, trailer descending),
 *        non-strictly: PBL_INVALID_ARG, as pbl_merge_batch;
 *      - a KV has PBL_KV_INVALID_KEY, or a kind other than the six above
 *        (visible or not; range keys and range deletions are out of scope, the
 *        rest is corruption to the reference): PBL_UNSUPPORTED;
 *      - without KEEP_OPERANDS, a chain of more than one operand holds a value
 *        that is a handle: PBL_UNSUPPORTED;
 *      - the block's result KVs reach 2^32, or its key or value bytes pass
 *        4 GiB: PBL_UNSUPPORTED.
 *     Where several apply, the first in this list is reported.
 *     PBL_KV_OBSOLETE is ignored: an obsolete point is shadowed by definition.
 *  6. Optional, per result KV: src_kv = the index in the input of the head (of
 *     the operand under KEEP_OPERANDS); n_src = the number of source KVs whose
 *     bytes the result value holds (under KEEP_OPERANDS: the chain's length at
 *     the chain's first KV, 0 at the others).
 *
 * The result has the layout of a decoded batch with one block per q, as a scan
 * or merge result (restarts unused, blk_rst_base zeros when given); everything
 * that reads a decoded batch reads it.  The input is as pbl_scan_batch takes a
 * batch (key_bytes / val_bytes readable 16 B past their end).
 *
 * Sizing and overflow as pbl_merge_*: pbl_visible_size writes blk_*_base,
 * blk_status and totals only; pbl_visible_batch does everything, and on a
 * capacity overflow writes every size, no bytes, and PBL_OVERFLOW in
 * totals.status_mask.  With PBL_VISIBLE_SIZED, pbl_visible_batch takes
 * statuses, sizes and roles from the workspace as the last pbl_visible_size
 * over the same input, snapshot and KEEP_OPERANDS left them.  The workspace
 * (DEVICE, 16-byte aligned, pbl_visible_workspace_bytes(n_blocks, n_kv)) serves
 * one call at a time; nothing in it scales with a group's length.  n_kv is the
 * batch's totals.n_kv as the host read it; a batch that holds more gives every
 * block PBL_INVALID_ARG.  All launches are stream-ordered.
 *
 * PBL_INVALID_ARG, before any device call: NULL in / out or a needed array,
 * comparer > PBL_CMP_CRDB, only one of the tiering arrays (in the input or in
 * the result), a workspace that is NULL, not 16-byte aligned or too short,
 * unknown flags (PBL_VISIBLE_SIZED is unknown to pbl_visible_size and to
 * pbl_visible_batch_host).
 */
#define PBL_SEQNUM_MAX ((1ull << 56) - 1)   /* base.SeqNumMax */
#define PBL_VISIBLE_SIZED 0x1u          /* pbl_visible_batch: statuses, sizes and roles are in the workspace */
#define PBL_VISIBLE_KEEP_OPERANDS 0x2u  /* rule 4 */

typedef struct pbl_visible_in {
  pbl_decode_out batch;  /* the arrays are DEVICE (HOST for pbl_visible_batch_host); capacities and workspace fields unused */
  uint32_t n_blocks, comparer /* PBL_CMP_* */;
  uint64_t n_kv;         /* see above; unused by pbl_visible_batch_host */
  uint64_t snapshot;
} pbl_visible_in;

typedef struct pbl_visible_out {
  pbl_decode_out result;  /* one block per q (see above); workspace fields unused */
  uint64_t* src_kv;       /* [result.kv_cap], optional */
  uint32_t* n_src;        /* [result.kv_cap], optional */
} pbl_visible_out;

uint64_t pbl_visible_workspace_bytes(uint32_t n_blocks, uint64_t n_kv);
int pbl_visible_size(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                     uint32_t flags, void* stream);
int pbl_visible_batch(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                      uint32_t flags, void* stream);
/* The same rules over arrays in HOST memory as the plain sequential state
 * machine (a different algorithm from the device's scan, so that the two check
 * each other).  No device call, no workspace, nothing read past a key's end.
 * Sizes, statuses, overflow rule and outputs as pbl_visible_batch.
 * Single-threaded. */
int pbl_visible_batch_host(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags);
/* sizeof(pbl_visible_in), its 5 field offsets, sizeof(pbl_visible_out), its 3
 * field offsets (the other layout lists are unchanged). */
size_t pbl_visible_struct_layout(uint64_t* out, size_t cap);

/* ---- range deletions in the read path, on the device ----
 * mergingIter skips a point k#s when some range tombstone [start, end)#t has
 * cmp(start, k) <= 0 && cmp(k, end) < 0, t visible at the snapshot and t > s
 * (isNextEntryDeleted, merging_iter.go:605; keyspan.Span.VisibleAt / CoversAt,
 * internal/keyspan/span.go:336, :396).  The reference applies t > s level by
 * level; under the LSM invariant (a deeper level holds no sequence number newer
 * than a shallower one) that equals the pure sequence-number rule, which is
 * what is built here: a KV is range-deleted iff
 *   max{t : tombstone visible at the snapshot and covering k} > s.
 * A point with s == t survives.  A tombstone is visible as a point is (rule 1
 * of the view above: t < snapshot, PBL_SEQNUM_MAX sees everything).
 *
 * A RUN is one table's range-deletion fragments as a decoded batch with ONE
 * block: what pbl_decode_batch (flags 0) produces from a row-format range-del
 * block (restart interval 1, no prefix sharing, rowblk_fragment_iter.go:116-139).
 * Per KV the key is the start user key, the trailer seq << 8 | 15
 * (InternalKeyKindRangeDelete), the value the end user key.  A valid run is
 * FRAGMENTED, as every sstable's is: KVs sorted by (start ascending under the
 * comparer, trailer descending); every fragment has start <= end (an empty one,
 * start == end, covers nothing; real tables hold such); two
 * consecutive fragments either have equal start and equal end, or
 * end_i <= start_{i+1}.  key_bytes and val_bytes must be readable 16 B past
 * their end, as for every source.
 *
 * pbl_rangedel_set flattens up to PBL_RANGEDEL_MAX_RUNS runs into the SET: a
 * decoded batch with one block whose KVs are the distinct boundary keys (every
 * start and every end of every run) ascending under the comparer.  Among
 * boundaries that compare equal the bytes are those of the first in (run,
 * fragment index, start before end) order.  Values are empty, kv_flags 0,
 * entry_off 0, and KV i has trailer cover_i << 8 | 15, cover_i the largest
 * visible t among the fragments of any run with start <= b_i < end, or 0 when
 * there is none (t = 0 covers nothing; the last boundary always has cover 0).
 * to_host(), the host iterator and the per-block seeks read the set unchanged.
 * No size call: at most 2T KVs and the runs' summed key and value bytes come
 * out (T = the runs' KVs), and a caller allocates those bounds; a smaller
 * capacity writes the sizes, no bytes, and PBL_OVERFLOW in totals.status_mask.
 * blk_status[0], the set being empty on any of them, in order of precedence:
 * the first run block status that is not PBL_OK, in run order; a kind other
 * than RANGEDEL, or PBL_KV_INVALID_KEY: PBL_UNSUPPORTED; a run that is not
 * fragmented as defined above, or that holds another number of KVs than
 * n_kv[r]: PBL_INVALID_ARG.  The workspace (DEVICE, 16-byte aligned,
 * pbl_rangedel_workspace_bytes(T)) serves one call at a time.  Stream-ordered,
 * no host synchronisation.
 *
 * pbl_rangedel_cover: for every KV of `batch` (n_blocks blocks, n_kv = its
 * totals.n_kv as the host read it), cover_seq[kv] (DEVICE [n_kv]) = the cover
 * of the last boundary <= the KV's user key, 0 before the first boundary.  An
 * empty set, or one whose blk_status[0] is not PBL_OK, gives all zeros, and so
 * does a KV of a block that is not PBL_OK.  The call is asynchronous like every
 * device entry point, so it cannot return the set's status: that stays in
 * set->blk_status[0] and set->totals->status_mask, which the caller of
 * pbl_rangedel_set reads once with the sizes.  One launch, no workspace.
 *
 * pbl_visible_size_rd / pbl_visible_batch_rd / pbl_visible_batch_host_rd are the
 * view above with rule 1 extended: a KV is visible iff trailer >> 8 < snapshot
 * and not cover_seq[kv] > trailer >> 8 (cover_seq: [in->n_kv] entries, DEVICE or
 * HOST as `in`; NULL = no range deletions, which is what the three entry points
 * above pass).  A range-deleted KV is an invisible KV everywhere: it heads no
 * group, is no operand and ends no MERGE chain.  Nothing else in the rules
 * changes.  With PBL_VISIBLE_SIZED the roles are the size call's and cover_seq
 * is not read again.
 *
 * The host forms take HOST arrays and use other algorithms, so that they and
 * the device check each other: pbl_rangedel_set_host sorts all boundaries
 * (std::stable_sort, unique) and takes a brute-force maximum over all
 * fragments per boundary; pbl_rangedel_cover_host takes the RUNS, not the set,
 * and brute-forces the maximum over every fragment per KV, so that it checks
 * the set builder and the lookup together; *status (optional) receives the
 * status the set would have.
 *
 * Levels.  The reference applies t > s level by level (isNextEntryDeleted): a
 * visible covering tombstone of a SHALLOWER level (a newer memtable, a newer L0
 * sublevel, a lower-numbered level) deletes a point whatever the two sequence
 * numbers are; one of the point's own level needs t > s.  In an LSM whose
 * sequence numbers are ordered by level the two forms agree; where a caller's
 * inputs may not be (testdata/range_del holds such memtables), it passes
 * levels: runs->level[r] for the tombstones, and to pbl_rangedel_cover_lv per
 * KV the run (table) it came from (src_run, DEVICE u8 [n_kv], what
 * pbl_merge_batch writes) and that run's level (run_level, HOST [16]).  The set
 * then holds in entry_off[i] (required with levels) 1 + the shallowest level
 * with a visible fragment covering b_i (0: none), and cover_seq[kv] is
 * PBL_RANGEDEL_ALL, above every sequence number, where that level is shallower
 * than the KV's, else the cover as above (a tombstone of a deeper level is
 * still judged by its sequence number).  Without levels (NULL) entry_off is 0
 * and the rule is the sequence-number one.  pbl_rangedel_cover is
 * pbl_rangedel_cover_lv with NULLs.
 *
 * PBL_INVALID_ARG, before any device call: NULL runs / set / batch / cover_seq
 * or a needed array, more than PBL_RANGEDEL_MAX_RUNS runs, runs->runs or
 * runs->n_kv NULL with n_runs > 0, comparer > PBL_CMP_CRDB, 2^31 fragments or
 * more, a workspace that is NULL, not 16-byte aligned or too short.
 */
#define PBL_RANGEDEL_MAX_RUNS 16
#define PBL_KIND_RANGEDEL 15u /* InternalKeyKindRangeDelete (internal/base/internal.go:29-130) */
#define PBL_RANGEDEL_ALL (1ull << 56) /* a cover above every sequence number: deleted by a shallower level */

typedef struct pbl_rangedel_runs {
  const pbl_decode_out* runs; /* HOST array [n_runs]; one block each; the arrays each names are DEVICE
                                 (HOST for the host forms); capacities and workspace fields unused */
  const uint64_t* n_kv;       /* HOST [n_runs]: each run's totals.n_kv as the host read it */
  uint32_t n_runs, comparer /* PBL_CMP_* */;
  uint64_t snapshot;
  const uint8_t* level;       /* HOST [n_runs] or NULL: each run's level, smaller = shallower (see "Levels") */
} pbl_rangedel_runs;

uint64_t pbl_rangedel_workspace_bytes(uint64_t n_fragments);
int pbl_rangedel_set(const pbl_rangedel_runs* runs, pbl_decode_out* set, void* workspace, uint64_t workspace_bytes,
                     void* stream);
int pbl_rangedel_set_host(const pbl_rangedel_runs* runs, pbl_decode_out* set);
int pbl_rangedel_cover(const pbl_decode_out* set, const pbl_decode_out* batch, uint32_t n_blocks, uint64_t n_kv,
                       uint32_t comparer, uint64_t* cover_seq, void* stream);
int pbl_rangedel_cover_host(const pbl_rangedel_runs* runs, const pbl_decode_out* batch, uint32_t n_blocks,
                            uint64_t* cover_seq, uint32_t* status);
int pbl_rangedel_cover_lv(const pbl_decode_out* set, const pbl_decode_out* batch, uint32_t n_blocks, uint64_t n_kv,
                          uint32_t comparer, const uint8_t* src_run, const uint8_t* run_level, uint64_t* cover_seq,
                          void* stream);
int pbl_rangedel_cover_host_lv(const pbl_rangedel_runs* runs, const pbl_decode_out* batch, uint32_t n_blocks,
                               const uint8_t* src_run, const uint8_t* run_level, uint64_t* cover_seq,
                               uint32_t* status);
int pbl_visible_size_rd(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                        uint32_t flags, const uint64_t* cover_seq, void* stream);
int pbl_visible_batch_rd(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                         uint32_t flags, const uint64_t* cover_seq, void* stream);
int pbl_visible_batch_host_rd(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags,
                              const uint64_t* cover_seq);
/* sizeof(pbl_rangedel_runs), its 6 field offsets (the other layout lists are
 * unchanged; ABI version 9 stands). */
size_t pbl_rangedel_struct_layout(uint64_t* out, size_t cap);

/* ---- columnar keyspan blocks, on the device --------------
 * A columnar table (Pebblev5 and later) keeps its range deletions, and its range
 * keys, in colblk keyspan blocks (sstable/colblk/keyspan.go).  These entry
 * points decode a batch of such blocks into RUNS as defined above: one result
 * block per input block, which pbl_rangedel_set, the host iterator and the
 * per-block seeks read unchanged.  batch->format, flags and block_format are
 * ignored; synthetic_seq_num applies (keyspan.go:599-603).
 *
 * Block layout (KeyspanDecoder.Init, keyspan.go:234-248): bytes 0-3 B, the
 * number of boundary user keys (LE32); from byte 4 the colblk header (custom
 * header size 4) with 5 columns and R rows, one per keyspan.Key; column 0
 * RawBytes with B rows, the boundary keys; column 1 Uint with B rows, idx[], the
 * first key row of the span that starts at each boundary; column 2 Uint with R
 * rows, the trailers; columns 3 and 4 RawBytes with R rows, the suffixes and the
 * values; one trailing padding byte.  Every DecodeColumn check applies, the end
 * of one column being the start of the next.
 *
 * The forward walk (First(); Next()...; keyspan.go:478-543): span s, 0 <= s <
 * B-1, is [boundary[s], boundary[s+1]) and holds key rows idx[s] .. idx[s+1]-1.
 * A span without rows is a gap and is passed over; an empty first span is
 * legal.  One KV comes out per key row j of span s: key = boundary[s], value =
 * boundary[s+1], trailer = column 2's word (or synthetic_seq_num << 8 | kind),
 * kv_flags 0, entry_off = j; there are no restarts (blk_rst_base all zero,
 * totals.n_restarts 0).  B < 2 is an OK block without KVs.  Rows before idx[0]
 * and from idx[B-1] on cannot be reached in the reference and are not output.
 *
 * blk_status: header or column directory failures, a column count other than
 * 5: PBL_CORRUPT_COLBLK_HEADER.  With B >= 2, PBL_CORRUPT_BOUNDS for: a boundary
 * offset that decreases; idx[s] > idx[s+1]; idx[B-1] > R; the last span empty;
 * two empty spans in a row; among the rows that are output, idx[0] .. idx[B-1]-1,
 * a suffix or value offset that decreases, or the end of the last such slice
 * (the offset of row idx[B-1]) past the column's own last offset, that of row
 * R, which is the only one DecodeColumn bounds (rows that no span reaches are
 * not looked at: the reference never reads them); B larger than the block's
 * length (its idx[] would be constant).  The reference finds these lazily, and panics on a decreasing or
 * out-of-range index; here they are reported for the whole block, which then
 * holds no KVs.  More than 4 GiB - 1 of key or of value bytes in one block:
 * PBL_UNSUPPORTED.  A block whose boundaries do not fit the workspace
 * (total_boundaries was too small): PBL_INVALID_ARG in blk_status.
 *
 * `extra` (optional, NULL allowed) receives per KV what a range key needs: the
 * start boundary index (span[kv]) and the keyspan.Key's Suffix and Value (not
 * the run's value, which is the end key), laid out as keys are: suffix j of
 * block b = suffix_bytes[blk_suffix_base[b] + suffix_off[o] .. + suffix_off[o+1])
 * with o = blk_kv_base[b] + b + j; likewise value_*.
 *
 * total_boundaries: the sum over the blocks of min(B, block_len), B being each
 * block's first four bytes (the caller reads them; a smaller number only makes
 * blocks PBL_INVALID_ARG).  The workspace (DEVICE, 16-byte aligned,
 * pbl_keyspan_workspace_bytes bytes) serves one call at a time.  The blocks
 * must be readable up to the next 16-byte boundary after every block, as for
 * every batch.  pbl_keyspan_size writes only blk_{kv,key,val,rst}_base,
 * blk_status and totals (and extra's two base arrays): exact sizes for the
 * allocation.  pbl_keyspan_decode writes everything; when a capacity is
 * exceeded (extra's included) it writes the sizes, no bytes, and PBL_OVERFLOW in
 * totals.status_mask.  key_off / val_off / suffix_off / value_off hold
 * kv_cap + n_blocks entries.  Stream-ordered, no host synchronisation.
 *
 * pbl_keyspan_decode_host is the same over HOST arrays by another algorithm:
 * the reference's sequential walk span by span (gatherKeysForward,
 * materializeSpan), with its own column decoders.  With out->key_off NULL it
 * sizes only.
 *
 * PBL_INVALID_ARG, before any device call: NULL batch / out or a needed array,
 * synthetic_seq_num >= 2^56, a workspace that is NULL, not 16-byte aligned or
 * too short.
 */
typedef struct pbl_keyspan_extra {
  uint32_t* span;            /* [kv_cap] the start boundary index of each KV's span */
  uint32_t* suffix_off;      /* [kv_cap + n_blocks] block-relative suffix offsets  */
  uint32_t* value_off;       /* [kv_cap + n_blocks] block-relative value offsets   */
  uint8_t* suffix_bytes;     /* [suffix_cap]                                       */
  uint8_t* value_bytes;      /* [value_cap]                                        */
  uint64_t* blk_suffix_base; /* [n_blocks+1]                                       */
  uint64_t* blk_value_base;  /* [n_blocks+1]                                       */
  uint64_t suffix_cap, value_cap;
} pbl_keyspan_extra;

uint64_t pbl_keyspan_workspace_bytes(uint32_t n_blocks, uint64_t total_boundaries);
int pbl_keyspan_size(const pbl_block_batch* batch, uint64_t total_boundaries, pbl_decode_out* out,
                     pbl_keyspan_extra* extra, void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_keyspan_decode(const pbl_block_batch* batch, uint64_t total_boundaries, pbl_decode_out* out,
                       pbl_keyspan_extra* extra, void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_keyspan_decode_host(const pbl_block_batch* batch, pbl_decode_out* out, pbl_keyspan_extra* extra);
/* sizeof(pbl_keyspan_extra), its 9 field offsets (the other layout lists are
 * unchanged; ABI version 9 stands). */
size_t pbl_keyspan_struct_layout(uint64_t* out, size_t cap);

/* ---- range keys in the read path --------------------------
 * What a bounded Iterator over several tables returns besides points: the range
 * keys in force at its snapshot (Iterator.RangeBounds / RangeKeys), and,
 * optionally, the points that those range keys mask (IterOptions.RangeKeyMasking).
 *
 * A range-key RUN is what pbl_keyspan_decode with `extra` produces from one
 * block: a decoded batch with ONE block, key = start, value = end, trailer kind
 * in {RANGEKEYSET 21, RANGEKEYUNSET 20, RANGEKEYDEL 19}, and per KV the
 * keyspan.Key's suffix and value in a pbl_keyspan_extra.  It is FRAGMENTED as
 * the runs of range deletions are (above), trailers descending inside a span.
 *
 * The rules (rangekey.CoalesceInto, internal/rangekey/coalesce.go:64-151;
 * UserIteratorConfig.Transform / ShouldDefragment,
 * internal/rangekeystack/user_iterator.go:148-241; keyspanimpl.MergingIter;
 * rangeKeyMasking.SpanChanged / SkipPoint, range_keys.go:259-362):
 *  merge     the runs are fragmented at every boundary of any run; an elementary
 *            interval holds the keys of every fragment that contains it, by
 *            trailer descending, ties by (run, index in the run);
 *  coalesce  a key is visible iff seq < snapshot (PBL_SEQNUM_MAX sees all); the
 *            visible keys whose trailer is greater than the largest visible
 *            RANGEKEYDEL trailer count (so at one sequence number a SET or UNSET
 *            is not cut by a DEL, kinds being 21 > 20 > 19); among those, keys
 *            whose suffixes compare equal under CompareRangeSuffixes
 *            (pbl_range_suffix_compare) are one group and its first key wins; a
 *            winner survives iff it is a SET; survivors by suffix ascending;
 *  defragment  two abutting intervals join when they hold the same non-zero
 *            number of survivors, suffixes pairwise compare-equal, values
 *            pairwise byte-equal; a joined span keeps the keys (suffix bytes,
 *            value bytes, trailers) of its leftmost interval; an interval
 *            without survivors is no span and breaks a chain;
 *  bounds    for [lower, upper) the spans that intersect it, the first one's
 *            start raised to lower, the last one's end lowered to upper;
 *  masking   with threshold suffix t: in the span covering a point k (start <=
 *            k < end) the mask is the smallest suffix r among the keys with a
 *            non-empty suffix and cmp(r, t) >= 0; k is masked iff its own suffix
 *            (k[split(k):]) is non-empty and cmp(r, p) < 0.  A masked KV is
 *            invisible everywhere, as a range-deleted one is.
 *
 * The SET is a decoded batch with ONE block and a pbl_keyspan_extra: one KV per
 * (span, surviving set), spans ascending, a span's KVs in suffix order.  Per KV:
 * key = the span's start, value = its end (among boundaries that compare equal
 * the bytes of the first in (run, fragment index, start before end) order),
 * trailer = the surviving set's, kv_flags 0, entry_off = the span's ordinal in
 * its block; extra: the key's suffix and value, and span[kv] = the index in the
 * block of the span's FIRST KV, which is how the mask reaches a span's keys with
 * one load (the ordinal is in entry_off already).  blk_status[0], the set being
 * empty on any of them, in order of precedence: the first run block status that
 * is not PBL_OK; a kind outside {19, 20, 21} or PBL_KV_INVALID_KEY:
 * PBL_UNSUPPORTED; a run that is not fragmented or holds another number of KVs
 * than n_kv[r]: PBL_INVALID_ARG.  4 GiB or more of key, end, suffix or value
 * bytes: PBL_UNSUPPORTED.  Sizes: an interval holds at most M = the sum over
 * the runs of a run's longest span (in keys) survivors and there are at most
 * 2T - 1 intervals (T = the runs' KVs), so at most (2T - 1) * M KVs come out,
 * each with a start, an end, a suffix and a value no longer than the longest of
 * the runs.  That bound is quadratic, so a caller offers what it expects; a
 * smaller capacity (extra's included) writes the sizes (totals, blk_*_base,
 * blk_suffix_base, blk_value_base), no bytes, and PBL_OVERFLOW in
 * totals.status_mask, and the caller calls again with those sizes.
 *
 * pbl_rangekey_set_host builds the set over HOST arrays in the reference's
 * sequential shape: it sorts the boundaries (std::stable_sort, unique), per
 * interval gathers the keys with one cursor per run (the merging iterator's
 * walk), sorts them by trailer, runs CoalesceInto and Transform literally, and
 * defragments in one left-to-right walk.  The set is small next to a batch: a caller builds it
 * once per read and copies it to the device for pbl_rangekey_mask (a device
 * builder is not built).
 *
 * pbl_rangekey_clip_host: a decoded batch (HOST) with one block per range of
 * `ranges` (HOST arrays; lower / upper keys, PBL_SCAN_NO_UPPER, n and comparer
 * are read; an empty lower key is below every key), holding the set's spans
 * that intersect the range, truncated to it, in the set's form with span[] and
 * entry_off relative to the block.  An empty or inverted range (upper <= lower)
 * intersects nothing: its block is empty.  Every block has the set's status.
 * to_host(), the host iterator and the per-block seeks read it unchanged.
 *
 * pbl_rangekey_mask: THE HOT PATH.  For every KV of `batch` (n_blocks blocks,
 * n_kv = its totals.n_kv as the host read it) that the masking rule hides under
 * the set (DEVICE arrays) and the threshold mask_suffix (DEVICE, readable 16 B
 * past its end; length 0 = the empty suffix, below every other), it stores
 * PBL_RANGEDEL_ALL into cover_seq[kv] (DEVICE [n_kv]).  Every other entry is
 * left as it is, so a cover from pbl_rangedel_cover composes with it (zero the
 * array first when there is none), and the _rd view applies the masking.  KVs
 * of blocks that are not PBL_OK are untouched; so is every KV when the set is
 * empty, not PBL_OK or overflowed.  One launch, no workspace, stream-ordered,
 * no host synchronisation.  The set's key, value and suffix bytes must be
 * readable 16 B past their end, as for every source.
 *
 * pbl_rangekey_mask_set_host is the same lookup over HOST arrays.
 * pbl_rangekey_mask_host takes the RUNS, not the set: per KV it gathers the
 * keys of every fragment that covers it, coalesces them and applies
 * SpanChanged / SkipPoint, so it checks the set builder and the lookup
 * together; *status (optional) receives the status the set would have (nothing
 * is stored with a status).
 *
 * PBL_INVALID_ARG, before anything else: NULL runs / set / extra / batch /
 * cover_seq / ranges or a needed array, more than PBL_RANGEDEL_MAX_RUNS runs,
 * runs->runs, runs->extras or runs->n_kv NULL with n_runs > 0, comparer >
 * PBL_CMP_CRDB, 2^31 fragments or more, mask_suffix NULL with a length.
 */
#define PBL_KIND_RANGEKEYDEL 19u   /* InternalKeyKindRangeKeyDelete (internal/base/internal.go:29-130) */
#define PBL_KIND_RANGEKEYUNSET 20u /* InternalKeyKindRangeKeyUnset */
#define PBL_KIND_RANGEKEYSET 21u   /* InternalKeyKindRangeKeySet   */

typedef struct pbl_rangekey_runs {
  const pbl_decode_out* runs;      /* HOST array [n_runs]; one block each; the arrays each names are DEVICE
                                      (HOST for the host forms); capacities and workspace fields unused */
  const pbl_keyspan_extra* extras; /* HOST array [n_runs]: each run's suffixes and values */
  const uint64_t* n_kv;            /* HOST [n_runs]: each run's totals.n_kv as the host read it */
  uint32_t n_runs, comparer /* PBL_CMP_* */;
  uint64_t snapshot;
} pbl_rangekey_runs;

/* Comparer.CompareRangeSuffixes: bytes.Compare (default), testkeys'
 * compareSuffixes, cockroachkvs.CompareRangeSuffixes: -1 / 0 / +1. */
int pbl_range_suffix_compare(uint32_t comparer, const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len);
int pbl_rangekey_set_host(const pbl_rangekey_runs* runs, pbl_decode_out* set, pbl_keyspan_extra* set_extra);
int pbl_rangekey_clip_host(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra, const pbl_scan_queries* ranges,
                           pbl_decode_out* out, pbl_keyspan_extra* out_extra);
int pbl_rangekey_mask(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra, const pbl_decode_out* batch,
                      uint32_t n_blocks, uint64_t n_kv, uint32_t comparer, const uint8_t* mask_suffix,
                      uint64_t mask_suffix_len, uint64_t* cover_seq, void* stream);
int pbl_rangekey_mask_set_host(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra,
                               const pbl_decode_out* batch, uint32_t n_blocks, uint32_t comparer,
                               const uint8_t* mask_suffix, uint64_t mask_suffix_len, uint64_t* cover_seq);
int pbl_rangekey_mask_host(const pbl_rangekey_runs* runs, const pbl_decode_out* batch, uint32_t n_blocks,
                           const uint8_t* mask_suffix, uint64_t mask_suffix_len, uint64_t* cover_seq,
                           uint32_t* status);
/* sizeof(pbl_rangekey_runs), its 6 field offsets (the other layout lists are
 * unchanged; ABI version 9 stands). */
size_t pbl_rangekey_struct_layout(uint64_t* out, size_t cap);

/* ---- table bloom filters: batched probes and SeekPrefixGE ----
 * The filter block of a table ("fullfilter.rocksdb.BuiltinBloomFilter" in the
 * metaindex; sstable/tablefilters/bloom): nLines * 64 bytes of bits, one byte
 * of probes, LE32 nLines -- the RocksDB full-file format.  The rules are
 * filter_core.hip.h's, stated once for host and device:
 *
 *   hash   bloom.go:41-78 over key[:Split(key)] under `comparer` (what a table's
 *          writer adds, and what Get / SeekPrefixGE ask for)
 *   parse  bits.go:93-105.  A filter of 5 bytes or fewer holds nothing: every
 *          probe answers "no", status PBL_OK.  nLines == 0, or a length that is
 *          not the one nLines gives (8 * ((len - 5) / nLines) != 512), is
 *          PBL_CORRUPT_FILTER (the reference panics).
 *   probe  bits.go:39-53: line h % nLines, nProbes bits of it, h += rotr(h, 17)
 *          between them.  nProbes is what the byte says (0 .. 255); zero probes
 *          answer "yes".
 *
 * pbl_filter_probe: one launch, a lane per key.  Named mode (q->filter != NULL):
 * key i against filter q->filter[i], may[i].  All-pairs mode (q->filter == NULL):
 * every key against every filter, hashed once, may[f * n + i].  may bits:
 * PBL_FILTER_MAY is the reference's MayContain; PBL_FILTER_BAD marks a filter id
 * >= n_filters or a corrupt filter, and then PBL_FILTER_MAY is set too: a caller
 * that ignores statuses must never lose a key (the entry points are
 * asynchronous: it cannot be a return code).  hash[i] (optional) is the hash of
 * key i's prefix; flt_status[f] (optional) the parse status of filter f.
 * off[] must be non-decreasing; filter f is bytes[off[f] .. off[f + 1]).
 *
 * PBL_INVALID_ARG, before any device call: a NULL struct, NULL may, NULL
 * key_off, comparer > PBL_CMP_CRDB.  n == 0 or n_filters == 0 returns PBL_OK
 * without a launch.
 *
 * pbl_filter_probe_host is the same over HOST pointers (single-threaded, no
 * device call, nothing read past a key's end).
 *
 * pbl_bloom_build_host is the writer (bloom.go:100-123, bits.go:73-89): the
 * hash of every key's Split-prefix in the order given, a hash equal to the one
 * before it dropped (hash_collector.go:39-42), nLines = ((numHashes *
 * bits_per_key + 511) / 512) | 1, the probe count of bloom.go:23-34.  Zero
 * hashes give *out_len = 0.  PBL_OVERFLOW (and the needed *out_len) when `cap`
 * is less than the filter; pbl_bloom_build_bound(n, bits_per_key) is always
 * enough.  bits_per_key == 0 is PBL_INVALID_ARG (FilterPolicy panics).  It
 * exists to make inputs and has no device form.
 */
#define PBL_FILTER_MAY 0x1u
#define PBL_FILTER_BAD 0x2u

typedef struct pbl_filter_set {      /* F filters, concatenated in one device buffer */
  const uint8_t*  bytes;             /* DEVICE */
  const uint64_t* off;               /* DEVICE [n_filters + 1] */
  uint32_t n_filters;
} pbl_filter_set;

typedef struct pbl_filter_queries {
  const uint8_t*  key_bytes;         /* DEVICE, readable 16 B past the last key */
  const uint64_t* key_off;           /* DEVICE [n + 1] */
  const uint32_t* filter;            /* DEVICE [n] one filter id per key, or NULL: every key against every filter */
  uint32_t n, comparer;              /* the probed bytes are key[:Split(key)] */
} pbl_filter_queries;

typedef struct pbl_filter_out {
  uint8_t*  may;        /* DEVICE [n] (named mode) or [n_filters * n], filter-major (all-pairs mode) */
  uint32_t* hash;       /* DEVICE [n], optional: bloom_hash of every key's prefix */
  int32_t*  flt_status; /* DEVICE [n_filters], optional: PBL_OK / PBL_CORRUPT_FILTER */
} pbl_filter_out;

int pbl_filter_probe(const pbl_filter_set* set, const pbl_filter_queries* q, pbl_filter_out* out, void* stream);
int pbl_filter_probe_host(const pbl_filter_set* set, const pbl_filter_queries* q, pbl_filter_out* out);
int pbl_bloom_build_host(const uint8_t* key_bytes, const uint64_t* key_off, uint64_t n, uint32_t comparer,
                         uint32_t bits_per_key, uint8_t* out, uint64_t cap, uint64_t* out_len);
uint64_t pbl_bloom_build_bound(uint64_t n, uint32_t bits_per_key);
/* sizeof(pbl_filter_set), its 3 field offsets, sizeof(pbl_filter_queries), its 5,
 * sizeof(pbl_filter_out), its 3 (the other layout lists are unchanged; ABI
 * version 9 stands: the additions change no existing struct or function). */
size_t pbl_filter_struct_layout(uint64_t* out, size_t cap);

/* singleLevelIterator.SeekPrefixGE with useFilterBlock
 * (sstable/reader_iter_single_lvl.go:1037-1107) in one launch: the prefix is the
 * query's own Split-prefix; a query whose prefix the filter excludes gets
 * PBL_SEEK_NONE, block 0 and flags PBL_SEEK_FILTERED, and its lane does no
 * search; every other query gets exactly what pbl_seek_batch gives it.  The
 * search is pbl_seek_batch's (seek_core.hip.h seek_one) behind that one
 * predicate.  `filter` is one filter block as above.  A corrupt filter excludes
 * nothing, and every answered query also carries PBL_SEEK_BAD_BLOCK.  Only
 * table mode (q->block == NULL) with PBL_SEEK_GE: anything else, or a NULL
 * filter, is PBL_INVALID_ARG, as is whatever pbl_seek_batch refuses.  A
 * synthetic prefix (bloomFilterMayContain, :1117-1126) is the caller's to strip.
 */
#define PBL_SEEK_FILTERED 0x8u   /* the table's filter excluded the key's prefix: kv = PBL_SEEK_NONE, no search ran */

int pbl_seek_prefix_batch(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_seek_queries* q,
                          const uint8_t* filter /* DEVICE */, uint64_t filter_len,
                          pbl_seek_out* out, const void* workspace, uint64_t workspace_bytes, void* stream);
int pbl_seek_prefix_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q,
                               const uint8_t* filter, uint64_t filter_len, pbl_seek_out* out);

/* ---- compaction view of a sorted decoded batch, on the device ----
 * What compact.Iter (internal/compact/iterator.go) returns over the point keys
 * of a block: not what a reader sees (pbl_visible_batch) but what a compaction
 * must KEEP.  Input as pbl_visible_batch takes it: one decoded batch whose
 * blocks are each sorted under (comparer, trailer descending); one comes out
 * with the same n_blocks, result block q being First(); Next()... of the
 * reference over block q with DefaultMerger.  Blocks are independent, there is
 * no visibility cut: every KV takes part.
 *
 *   snapshots   ascending sequence numbers, any number including none
 *   PBL_COMPACT_ELIDE_TOMBSTONES  ElideTombstonesOutsideOf(nil): every point
 *                                 tombstone may be elided
 *   PBL_COMPACT_BOTTOMMOST        IterConfig.IsBottommostDataLayer
 *
 * Stripes and segments.  A KV's stripe is Snapshots.Index(seq), the number of
 * snapshots <= seq (snapshots.go:50-54).  A segment is a maximal run of KVs of
 * a block with equal user key (key_cmp == 0) and equal stripe.  The iterator's
 * state never crosses a segment boundary (nextInStripe, iterator.go:778-851).
 * Inside a segment the reference processes a HEAD, which decides what happens
 * to the KVs after it; below, "elided" means ELIDE_TOMBSTONES and stripe 0,
 * "tombstone" one of DEL / SINGLEDEL / DELSIZED, and "the rest is skipped"
 * that no later KV of the segment is a head (skipInStripe, :726-737).  A DEL's
 * and a SINGLEDEL's value bytes are never read: they are value-less (:605,
 * :1010).
 *
 * Head rules (Iter.Next, :439-704):
 *  DEL / DELSIZED, elided (:576-593): nothing is emitted, the rest is skipped.
 *  SINGLEDEL, elided (skipDueToSingleDeleteElision, :1099-1185): nothing is
 *     emitted.  The next KV of the segment: a SINGLEDEL repeats the rule (one
 *     ineffectual call); DEL / DELSIZED (one ineffectual call) and SETWITHDEL
 *     skip the rest; a SET / MERGE is consumed and the KV after it is a fresh
 *     head.  The segment ending on the pending SINGLEDEL: one ineffectual call.
 *  DEL otherwise (:603-607): emitted with an empty value; the rest is skipped.
 *  SET (setNext, :853-905): emitted with its own value; the kind becomes
 *     SETWITHDEL iff a tombstone follows anywhere in the segment; the rest is
 *     skipped.  SETWITHDEL: emitted as it is; the rest is skipped.
 *  MERGE (mergeNext, :907-992): the following MERGEs of the segment are
 *     operands; a SET / SETWITHDEL is the last operand and makes the kind SET; a
 *     tombstone ends the chain without being an operand and makes the kind
 *     SETWITHDEL; a chain that reaches the segment's end stays MERGE.  The
 *     value is the operands' values concatenated OLDEST FIRST, as
 *     pbl_visible_batch.  The rest is skipped.
 *  SINGLEDEL otherwise (singleDeleteNext, :1004-1087): the next KV of the
 *     segment decides.  None: emitted as SINGLEDEL.  DEL / DELSIZED (one
 *     ineffectual call) or SETWITHDEL: emitted with kind DEL and its own
 *     sequence number, the rest is skipped.  SINGLEDEL: one ineffectual call, it
 *     is passed over and the FIRST one's key and trailer are kept.  SET / MERGE:
 *     consumed together with it, nothing is emitted, and the KV after it is a
 *     fresh head.
 *     After a consumed SET / MERGE (elided or not), a next KV of the same user
 *     key (in any stripe) of kind SET / SETWITHDEL / MERGE is one
 *     nondeterministic call (:1049-1073, :1151-1176).
 *  DELSIZED otherwise (deleteSizedNext, :1193-1363): emitted; it holds a value,
 *     at first its own.  Every following KV of the segment:
 *       a tombstone: if the held value is not empty, one missized DELSIZED; the
 *         held value becomes that KV's (empty for DEL / SINGLEDEL); a DEL or
 *         SINGLEDEL makes the kind DEL and the rest is skipped;
 *       SET / MERGE / SETWITHDEL with an empty held value: kind DEL, the rest is
 *         skipped;
 *       the same with a held value: it is one uvarint, the expected size; if
 *         len(that KV's user key) + len(its value) differs, one missized
 *         DELSIZED, kind DEL, empty value, the rest is skipped; if it matches,
 *         the held value becomes empty and the walk goes on.
 *     The result's value is the held value at the segment's end.  A held value
 *     that is not exactly one uvarint where the reference decodes it (:1249,
 *     :1308: at any following KV) is corruption: PBL_CORRUPT_BOUNDS.
 *  With PBL_COMPACT_BOTTOMMOST in stripe 0 (:659-666, :862-864): an emitted SET /
 *     SETWITHDEL / MERGE head gets sequence number 0, and a MERGE that stayed
 *     MERGE becomes SET.
 *
 * A result KV carries the head's key bytes, the rewritten trailer, the value
 * as above, and the head's entry_off, tiering meta and value-kind flag bits, as
 * the visible view does.  Optional outputs per result KV: src_kv (the head's
 * index in the input), n_src (the operands of a MERGE chain, 1 otherwise) and
 * pinned (Iter.SnapshotPinned(), :392, :482, :598): 1 when the head starts its
 * segment and the KV before it has the same user key, or when the head is a
 * tombstone, ELIDE_TOMBSTONES is set and its stripe is not 0.  Optional outputs
 * per block, zero for a block that is not PBL_OK: n_missized
 * (IterStats.CountMissizedDels), n_ineffectual and n_nondeterministic (the
 * calls of IneffectualSingleDeleteCallback / NondeterministicSingleDeleteCallback).
 *
 * Statuses: a result block is empty, its neighbours unaffected, when (first
 * that applies)
 *   - the input block is not PBL_OK: that status;
 *   - the block is not sorted; two KVs of one user key with equal sequence
 *     numbers count as not sorted (:817-822): PBL_INVALID_ARG;
 *   - a KV has PBL_KV_INVALID_KEY or a kind outside the six; a value that is a
 *     handle takes part in a MERGE chain of more than one operand:
 *     PBL_UNSUPPORTED;
 *   - a DELSIZED value as above: PBL_CORRUPT_BOUNDS;
 *   - the result's KVs reach 2^32 or its key or value bytes pass 4 GiB:
 *     PBL_UNSUPPORTED.
 * PBL_KV_OBSOLETE is ignored.
 *
 * Sizing, overflow, workspace and n_kv as pbl_visible_*; with PBL_COMPACT_SIZED
 * pbl_compact_batch takes everything from the workspace as the last
 * pbl_compact_size over the same input, snapshots and flags left it.
 * PBL_INVALID_ARG before any device call as there, and for unknown flags
 * (PBL_COMPACT_SIZED is unknown to pbl_compact_size and the host form) and
 * n_snapshots != 0 with a NULL list.  The snapshot list is DEVICE memory for
 * the device calls, which cannot see its order; the host form checks that it
 * ascends (non-strictly) and answers PBL_INVALID_ARG otherwise.
 *
 * Out of scope: range deletions and range keys in the stream,
 * elision by key ranges, user and deletable mergers, blob values in chains,
 * output splitting.
 */
#define PBL_COMPACT_SIZED 0x1u             /* pbl_compact_batch: the workspace holds the last pbl_compact_size */
#define PBL_COMPACT_ELIDE_TOMBSTONES 0x2u
#define PBL_COMPACT_BOTTOMMOST 0x4u

typedef struct pbl_compact_in {
  pbl_decode_out batch;  /* the arrays are DEVICE (HOST for pbl_compact_batch_host); capacities and workspace fields unused */
  uint32_t n_blocks, comparer /* PBL_CMP_* */;
  uint64_t n_kv;              /* as pbl_visible_in; unused by pbl_compact_batch_host */
  const uint64_t* snapshots;  /* [n_snapshots] ascending; DEVICE (HOST for the host form) */
  uint64_t n_snapshots;
} pbl_compact_in;

typedef struct pbl_compact_out {
  pbl_decode_out result;  /* one block per q; workspace fields unused */
  uint64_t* src_kv;       /* [result.kv_cap], optional */
  uint32_t* n_src;        /* [result.kv_cap], optional */
  uint8_t* pinned;        /* [result.kv_cap], optional */
  uint32_t* n_missized;          /* [n_blocks], optional */
  uint32_t* n_ineffectual;       /* [n_blocks], optional */
  uint32_t* n_nondeterministic;  /* [n_blocks], optional */
} pbl_compact_out;

uint64_t pbl_compact_workspace_bytes(uint32_t n_blocks, uint64_t n_kv);
int pbl_compact_size(const pbl_compact_in* in, pbl_compact_out* out, void* workspace, uint64_t workspace_bytes,
                     uint32_t flags, void* stream);
int pbl_compact_batch(const pbl_compact_in* in, pbl_compact_out* out, void* workspace, uint64_t workspace_bytes,
                      uint32_t flags, void* stream);
/* The same rules over HOST arrays as the sequential loop of the reference's
 * shape (a different algorithm from the device's scans, so that the two check
 * each other).  No device call, no workspace.  Single-threaded. */
int pbl_compact_batch_host(const pbl_compact_in* in, pbl_compact_out* out, uint32_t flags);
/* sizeof(pbl_compact_in), its 6 field offsets, sizeof(pbl_compact_out), its 7
 * (the other layout lists are unchanged; ABI version 9 stands). */
size_t pbl_compact_struct_layout(uint64_t* out, size_t cap);

/* ---- row-block encoder: a sorted decoded batch back into data blocks ----
 * The write side of the row format as a batch operation: a decoded batch goes
 * in, finished row-format data blocks come out, cut where Pebble's table writer
 * cuts them and byte for byte what RawRowWriter + rowblk.Writer produce
 * (sstable/rowblk/rowblk_writer.go:128-320; RawRowWriter.addPoint /
 * makeAddPointDecisionV3 / shouldFlush, sstable/rowblk_writer.go:585-774,
 * :1238-1262; FlushGovernor without size classes,
 * sstable/block/flush_governor.go:103-143).
 *
 * Block q of the input is one STREAM: an independent sorted sequence of KVs
 * (one range of a compact_tables result, say).  Every stream is encoded as if
 * by a fresh table writer and its output blocks are consecutive.  A stream
 * without KVs, or whose blk_status is not PBL_OK, produces no blocks;
 * stream_status[q] carries the input status.  Input values carry no value
 * prefix byte (what a decode with PBL_ROW_VALUE_PREFIX | PBL_ROW_NO_VALUER
 * yields).  "Predecessor" below is the previous KV of the stream, whichever
 * block it went to.
 *
 * Options: restart_interval ri >= 1; target_block_size in [1, 2^31);
 * block_size_threshold (percent); comparer (PBL_CMP_*: Split and Compare);
 * flags PBL_ENC_VALUE_PREFIX (TableFormat >= Pebblev3), PBL_ENC_OBSOLETE
 * (>= Pebblev4; without VALUE_PREFIX: PBL_INVALID_ARG), PBL_ENC_LOWEST_LEVEL
 * (writingToLowestLevel).  low = (target * threshold + 99) / 100, high = target.
 *
 *  1 Internal key = user key || LE64(trailer); a KV written obsolete has the
 *    trailer OR-ed with the obsolete bit (64) first.
 *  2 Shared prefix.  Entries 0, ri, 2 ri, ... OF THEIR BLOCK are restarts and
 *    share 0 bytes.  Any other entry shares the common prefix of its internal
 *    key and its predecessor's, capped at min(max_shared, both lengths).
 *    Without VALUE_PREFIX max_shared = len(user key), so that a predecessor
 *    whose user key is shorter lets the comparison run into its trailer bytes
 *    ("k"#..,SET before "k\x01.." shares 2 bytes): internal-key bytes are
 *    compared, not user keys.  With VALUE_PREFIX max_shared = Split(the
 *    predecessor's user key).
 *  3 set_same(k), with VALUE_PREFIX: k has a predecessor, both kinds are SET and
 *    Compare(prev[:Split(prev)], cur[:Split(cur)]) == 0.  A SET's stored value
 *    is the byte InPlaceValuePrefix(set_same) (0x00 / 0x20, sstable/block/
 *    kv.go:75-81) and then the value; every other kind stores the value bare.
 *    Without the flag set_same is false and nothing is prefixed.  Value blocks
 *    are not built: every value is stored in place.
 *  4 Obsolete, with OBSOLETE:
 *      obs(k) = force(k) || (pred(k) && C3(k)) ||
 *               (same_user_key(k) && (obs(k-1) || kind(k-1) != MERGE))
 *    force = the input's PBL_KV_OBSOLETE flag (forceObsolete); C3 =
 *    LOWEST_LEVEL and kind in {DEL, SINGLEDEL, DELSIZED}; pred(k): k has a
 *    predecessor (makeAddPointDecisionV3 returns before C3 for a table's first
 *    point key, :590-592); same_user_key: Compare == 0 with the predecessor.
 *    Without the flag nothing is written obsolete and input flags are ignored.
 *  5 Entry = uvarint(shared) uvarint(len(ikey) - shared) uvarint(len(stored
 *    value)) ikey[shared:] stored value.
 *  6 Restart word r of a block = the offset of block entry r * ri; bit 31 is set
 *    iff r >= 1 and set_same held for each of the entries (r-1) ri + 1 .. r ri.
 *    Restart 0 never has it (the table writer resets the block writer).  Block
 *    tail: the restart words, then their count, LE32 each.
 *  7 Flush.  With S(i, j) = EstimatedSize of the block of stream KVs i .. j-1
 *    (entry bytes + 4 per restart + 4), the block that starts at KV i ends
 *    before the first j > i for which
 *      S(i, j) >= low  and
 *      S(i, j) + len(ikey_j) + len(stored value_j) + (4 if (j - i) % ri == 0)
 *        + 4 + uvarint_len(len(ikey_j)) + uvarint_len(len(stored value_j)) > high
 *    (the reference's overestimate: 4 bytes for the shared varint, the whole
 *    key).  A block below low takes the next KV however large.
 *  8 Key order is not checked (disableKeyOrderChecks): the input is sorted by
 *    contract.  With target < 2^31 no block's entry area reaches 2^31 bytes
 *    before its last entry, so ErrBlockTooBig cannot arise; a stream holding a
 *    KV whose entry alone is 2^31 bytes or more is PBL_UNSUPPORTED (its block
 *    length would not fit 32 bits) and produces no blocks.
 *
 * Outputs (caller-allocated; DEVICE, HOST for the host form):
 *   blocks            block b at blocks[block_off[b] .. + block_len[b]); block_off
 *                     is 16-byte aligned, blocks follow each other, and the bytes
 *                     from a block's end to the next 16-byte boundary are zero: the
 *                     three arrays are a pbl_block_batch for pbl_decode_batch
 *   block_stream, block_first_kv (index into the batch's KV arrays), block_n_kv
 *                     what an index entry is made of: the block's last key is KV
 *                     first + n - 1, the next block's first key KV first + n
 *   stream_block_base [n_streams + 1]: stream q's blocks are [base[q], base[q+1])
 *   stream_status     [n_streams]
 *   obsolete          [n_kv], optional: the bit each KV was written with (0 for
 *                     KVs of streams that produced nothing)
 *   totals            blocks, bytes of `blocks` needed (a multiple of 16),
 *                     restart words, OR of (1u << status) over streams that are
 *                     not OK, and their number
 * pbl_rowenc_size writes totals, stream_block_base and stream_status only (the
 * other pointers and the capacities are ignored) and leaves the partition in
 * the workspace; pbl_rowenc_batch with PBL_ROWENC_SIZED takes it from there
 * (same input, options and workspace), without it computes it first.  When
 * n_blocks > block_cap or block_bytes > blocks_cap every size is still written
 * (totals, stream_block_base, stream_status), totals.status_mask has
 * 1u << PBL_OVERFLOW, and the block arrays and bytes are unspecified.  in->n_kv
 * is the batch's totals.n_kv as the host read it (below 2^32 - 1).  The
 * workspace is DEVICE memory, 16-byte aligned, of pbl_rowenc_workspace_bytes.
 * PBL_INVALID_ARG before any device call: NULL arguments, an input batch that
 * lacks an array the rules read, options out of range, unknown flags, a short
 * or misaligned workspace.
 */
#define PBL_ENC_VALUE_PREFIX 0x1u
#define PBL_ENC_OBSOLETE 0x2u
#define PBL_ENC_LOWEST_LEVEL 0x4u
#define PBL_ROWENC_SIZED 0x1u /* pbl_rowenc_batch flags: the workspace holds the last pbl_rowenc_size */

typedef struct pbl_rowenc_opts {
  uint32_t restart_interval;
  uint32_t target_block_size;
  uint32_t block_size_threshold; /* percent */
  uint32_t comparer;             /* PBL_CMP_* */
  uint32_t flags;                /* PBL_ENC_* */
  uint32_t reserved;
} pbl_rowenc_opts;

typedef struct pbl_rowenc_in {
  pbl_decode_out batch; /* the arrays are DEVICE (HOST for the host form); capacities and workspace fields unused */
  uint32_t n_streams;   /* the batch's blocks */
  uint32_t reserved;
  uint64_t n_kv;        /* unused by pbl_rowenc_batch_host */
} pbl_rowenc_in;

typedef struct pbl_rowenc_totals {
  uint64_t n_blocks;
  uint64_t block_bytes;
  uint64_t n_restarts;
  uint32_t status_mask;
  uint32_t n_bad_streams;
} pbl_rowenc_totals;

typedef struct pbl_rowenc_out {
  uint8_t* blocks;             /* [blocks_cap] */
  uint64_t* block_off;         /* [block_cap] */
  uint32_t* block_len;         /* [block_cap] */
  uint32_t* block_stream;      /* [block_cap] */
  uint64_t* block_first_kv;    /* [block_cap] */
  uint32_t* block_n_kv;        /* [block_cap] */
  uint64_t* stream_block_base; /* [n_streams + 1] */
  uint32_t* stream_status;     /* [n_streams] */
  uint8_t* obsolete;           /* [n_kv], optional */
  pbl_rowenc_totals* totals;   /* [1] */
  uint64_t blocks_cap, block_cap;
} pbl_rowenc_out;

uint64_t pbl_rowenc_workspace_bytes(uint32_t n_streams, uint64_t n_kv);
int pbl_rowenc_size(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out, void* workspace,
                    uint64_t workspace_bytes, void* stream);
int pbl_rowenc_batch(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out, void* workspace,
                     uint64_t workspace_bytes, uint32_t flags, void* stream);
/* The same rules over HOST arrays as the reference's sequential loop: one
 * pbl_rowblk_writer per block and shouldFlush before every Add (a different
 * algorithm from the device's scans, so that the two check each other).  No
 * device call, no workspace.  Single-threaded. */
int pbl_rowenc_batch_host(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out);
/* sizeof(pbl_rowenc_opts), its 6 field offsets, sizeof(pbl_rowenc_in), its 4,
 * sizeof(pbl_rowenc_totals), its 5, sizeof(pbl_rowenc_out), its 12 (the other
 * layout lists are unchanged; ABI version 9 stands). */
size_t pbl_rowenc_struct_layout(uint64_t* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PEBBLE_AMD_H */
