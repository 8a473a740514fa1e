"""Whole tables to decoded blocks on the device.

`Table` mirrors what sstable.Reader does at open and at iteration
(sstable/reader.go:1160-1260, table.go:298-404): read the footer, the
metaindex and the properties, load the index, walk its handles to the data
blocks.  Every block step runs in libpebble_amd.so:

  footer          pbl_parse_footer (host: the last 61 bytes of the file)
  metaindex       physical step (pbl_verify_checksums, pbl_decompress_blocks),
                  then a colblk KeyValueBlock (pbl_kv_blocks) for Pebblev6+
                  (reader.go:536-545, layout.go:789-824) or a row block decoded
                  with PBL_ROW_RAW_KEYS before that (layout.go decodeMetaindex)
  properties      the same two block kinds, KeyValueBlock from Pebblev7 on
                  (reader.go:601-617).  "rocksdb.block.based.table.index.type"
                  (LE32, properties_gen.go:96-98) decides single- or two-level
                  (Properties.toAttributes, properties.go:221-223; a Pebblev7
                  footer's AttributeTwoLevelIndex bit must agree,
                  reader.go:1214-1221); "pebble.colblk.schema" picks the
                  columnar key schema ("crdb1" = cockroachkvs.KeySchema,
                  "DefaultKeySchema(<comparer>,<bundle>)" = colblk.DefaultKeySchema,
                  reader.go:1244-1254)
  index blocks    physical step, then pbl_index_handles_row (row formats, after
                  pbl_decode_batch) or pbl_index_handles_col (columnar formats);
                  two-level tables run the step twice, the top level's handles
                  becoming the second-level batch's offsets
  data blocks     the handles become a PhysBatch over the file bytes already
                  in HBM: checksums, decompression, then `batch.decode`

The index's handles never visit the host on the data path: they are device
arrays that become the next batch's offsets.  Only the metaindex and the
properties -- a few hundred bytes the reader also keeps on the host -- are
read back.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .batch import BlockBatch, DecodedBatch, DecodeError, _stream_handle, decode
from .physical import PhysBatch, decompress, verify_checksums

MAX_FOOTER_LEN = 61  # table.go maxFooterLen (Pebblev7+)
TWO_LEVEL_INDEX = 2  # table.go twoLevelIndex
ATTRIBUTE_TWO_LEVEL_INDEX = 1 << 5  # attributes.go:13-18
INDEX_TYPE_PROP = b"rocksdb.block.based.table.index.type"
KEY_SCHEMA_PROP = b"pebble.colblk.schema"
PROPERTIES_NAME = b"rocksdb.properties"
VALUE_INDEX_NAME = b"pebble.value_index"
RANGE_DEL_NAME = b"rocksdb.range_del2"  # table.go metaRangeDelV2Name
RANGE_KEY_NAME = b"pebble.range_key"    # table.go metaRangeKeyName (sstable/table.go:229)
COMPARER_PROP = b"rocksdb.comparator"
COMPARERS = {b"leveldb.BytewiseComparator": N.PBL_CMP_DEFAULT, b"pebble.internal.testkeys": N.PBL_CMP_TESTKEYS,
             b"cockroach_comparator": N.PBL_CMP_CRDB}


@dataclass
class Footer:
    table_format: int
    checksum_type: int
    metaindex: tuple
    index: tuple
    footer: tuple
    attributes: int

    @property
    def columnar(self) -> bool:
        return self.table_format >= N.PBL_TABLE_PEBBLEV5  # Pebblev5+ (format.go BlockColumnar)


def parse_footer(tail: bytes, file_size: int) -> Footer:
    """parseFooter over the last bytes of a file (pbl_parse_footer)."""
    f = N.FooterC()
    rc = N.lib().pbl_parse_footer(bytes(tail), len(tail), file_size, ctypes.byref(f))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_parse_footer: {N.STATUS_NAMES.get(rc, rc)}")
    return Footer(f.table_format, f.checksum_type, (f.metaindex_off, f.metaindex_len), (f.index_off, f.index_len),
                  (f.footer_off, f.footer_len), f.attributes)


@dataclass
class IndexHandles:
    handle_off: torch.Tensor  # int64 (u64) [n]
    handle_len: torch.Tensor  # int64 (u64) [n]
    props_off: torch.Tensor   # int64 [n]
    props_len: torch.Tensor   # int32 [n]
    blk_base: torch.Tensor    # int64 [n_blocks + 1]
    blk_status: torch.Tensor  # int32 [n_blocks]

    def c_struct(self) -> N.IndexOutC:
        return N.IndexOutC(self.handle_off.data_ptr(), self.handle_len.data_ptr(), self.props_off.data_ptr(),
                           self.props_len.data_ptr(), self.blk_base.data_ptr(), self.blk_status.data_ptr(),
                           self.handle_off.numel())

    @classmethod
    def allocate(cls, n_blocks: int, cap: int, device) -> "IndexHandles":
        e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=device)  # noqa: E731
        return cls(e(cap, torch.int64), e(cap, torch.int64), e(cap, torch.int64), e(cap, torch.int32),
                   e(n_blocks + 1, torch.int64), e(n_blocks, torch.int32))

    def status(self) -> np.ndarray:
        return self.blk_status.cpu().numpy().view(np.uint32)

    def total(self, n_blocks: int) -> int:
        return int(self.blk_base[n_blocks].item())


def index_handles_row(decoded: DecodedBatch, n_blocks: int, stream=None) -> IndexHandles:
    """rowblk.IndexIter.BlockHandleWithProperties of every entry of decoded row
    index blocks (pbl_index_handles_row)."""
    n = int(decoded.read_totals().n_kv)
    out = IndexHandles.allocate(n_blocks, n, decoded.trailer.device)
    c = out.c_struct()
    o = decoded.c_struct()
    rc = N.lib().pbl_index_handles_row(ctypes.byref(o), n_blocks, ctypes.byref(c), _stream_handle(stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_index_handles_row: {N.STATUS_NAMES.get(rc, rc)}")
    return out


def index_handles_col(batch: BlockBatch, cap: Optional[int] = None, stream=None) -> IndexHandles:
    """colblk.IndexIter handles of raw columnar index blocks
    (pbl_index_handles_col); re-runs once with the exact size on overflow."""
    cap = cap if cap is not None else max(1, batch.input_bytes() // 4)
    for _ in range(2):
        out = IndexHandles.allocate(batch.n_blocks, cap, batch.device)
        c = out.c_struct()
        b = batch.c_struct()
        rc = N.lib().pbl_index_handles_col(ctypes.byref(b), ctypes.byref(c), _stream_handle(stream))
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_index_handles_col: {N.STATUS_NAMES.get(rc, rc)}")
        tot = out.total(batch.n_blocks)
        if tot <= cap:
            return out
        cap = tot
    return out


@dataclass
class KvSlices:
    """colblk.KeyValueBlockDecoder KeyAt/ValueAt of every row of a batch of
    key-value blocks, as slices of the batch's bytes (pbl_kv_blocks)."""
    key_off: torch.Tensor     # int64 (u64) [n]
    key_len: torch.Tensor     # int32 [n]
    val_off: torch.Tensor     # int64 (u64) [n]
    val_len: torch.Tensor     # int32 [n]
    blk_base: torch.Tensor    # int64 [n_blocks + 1]
    blk_status: torch.Tensor  # int32 [n_blocks]

    def c_struct(self) -> N.KvOutC:
        return N.KvOutC(self.key_off.data_ptr(), self.key_len.data_ptr(), self.val_off.data_ptr(),
                        self.val_len.data_ptr(), self.blk_base.data_ptr(), self.blk_status.data_ptr(),
                        self.key_off.numel())

    def status(self) -> np.ndarray:
        return self.blk_status.cpu().numpy().view(np.uint32)


def kv_blocks(batch: BlockBatch, cap: Optional[int] = None, stream=None) -> KvSlices:
    """pbl_kv_blocks over a batch of colblk key-value blocks; re-runs once with
    the exact size on overflow."""
    cap = cap if cap is not None else max(1, batch.input_bytes() // 4)
    for _ in range(2):
        e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=batch.device)  # noqa: E731
        out = KvSlices(e(cap, torch.int64), e(cap, torch.int32), e(cap, torch.int64), e(cap, torch.int32),
                       e(batch.n_blocks + 1, torch.int64), e(batch.n_blocks, torch.int32))
        c = out.c_struct()
        b = batch.c_struct()
        rc = N.lib().pbl_kv_blocks(ctypes.byref(b), ctypes.byref(c), _stream_handle(stream))
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_kv_blocks: {N.STATUS_NAMES.get(rc, rc)}")
        tot = int(out.blk_base[batch.n_blocks].item())
        if tot <= cap:
            return out
        cap = tot
    return out


def resolve_values(d: DecodedBatch, value_blocks: BlockBatch, stream=None) -> DecodedBatch:
    """pbl_resolve_values: every value-block handle of `d` replaced by the value
    it names in `value_blocks` (valueBlockFetcher.Fetch, valblk/reader.go:251-302).
    Returns a DecodedBatch sharing `d`'s keys and trailers with new values,
    per-block statuses and totals."""
    nb = d.n_blocks
    st = stream if stream is not None else torch.cuda.current_stream(d.trailer.device)
    cap = int(d.cap.val) + value_blocks.input_bytes() + 16
    for _ in range(2):
        with torch.cuda.stream(st):
            e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=d.trailer.device)  # noqa: E731
            vo, vbytes = e(d.val_off.numel(), torch.int32), e(cap + 16, torch.uint8)
            base, bst = e(nb + 1, torch.int64), e(nb, torch.int32)
        c = N.ValueOutC(vo.data_ptr(), vbytes.data_ptr(), base.data_ptr(), bst.data_ptr(), cap)
        o = d.c_struct()
        vb = value_blocks.c_struct()
        rc = N.lib().pbl_resolve_values(ctypes.byref(o), nb, ctypes.byref(vb), ctypes.byref(c),
                                        ctypes.c_void_p(st.cuda_stream))
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_resolve_values: {N.STATUS_NAMES.get(rc, rc)}")
        st.synchronize()
        tot = int(base[nb].item()) if nb else 0
        if tot <= cap:
            break
        cap = tot
    t = d.read_totals()
    status = bst.cpu().numpy().view(np.uint32)
    mask = 0
    for x in set(status.tolist()):
        mask |= (1 << x) if x else 0
    t2 = N.TotalsC(t.n_kv, t.key_bytes, tot, t.n_restarts, mask, int((status != 0).sum()), t.n_slow_blocks, 0)
    totals = torch.frombuffer(bytearray(bytes(t2)), dtype=torch.uint8).to(d.trailer.device)
    from dataclasses import replace
    from .batch import Capacity
    cap2 = Capacity(d.cap.kv, d.cap.key, cap, d.cap.rst)
    return replace(d, val_off=vo, val_bytes=vbytes, blk_val_base=base, blk_status=bst, totals=totals, cap=cap2,
                   _host_totals=None)


def _uvarint(b: bytes, i: int = 0):
    x = s = 0
    while True:
        c = b[i]
        x |= (c & 0x7F) << s
        i += 1
        if c < 0x80:
            return x, i
        s += 7


class Table:
    """One SST whose bytes are resident on a device."""

    def __init__(self, data, device="cuda"):
        host = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        self.size = len(host)
        self.footer = parse_footer(host[max(0, self.size - MAX_FOOTER_LEN):].tobytes(), self.size)
        pad = np.zeros(self.size + 16, np.uint8)
        pad[: self.size] = host
        self.bytes = torch.from_numpy(pad).to(device)
        self.device = self.bytes.device
        self._meta = None
        self._meta_raw = None
        self._props = None
        self._seek = None
        self._scan = {}
        self._filter = False  # not read yet (None: the table has no bloom filter)

    # -- the physical step for any set of handles already on the device ----------
    def _blocks(self, off: torch.Tensor, length: torch.Tensor, fmt: int, flags: int = 0) -> BlockBatch:
        pb = PhysBatch(self.bytes, off.contiguous(), length.to(torch.int32).contiguous())
        st, _ = verify_checksums(pb, self.footer.checksum_type)
        if st.any():
            raise DecodeError(f"block checksum mismatch in {int((st != 0).sum())} block(s)")
        bb, st = decompress(pb, fmt, flags)
        if st.any():
            raise DecodeError(f"decompression failed: {sorted(set(N.STATUS_NAMES.get(int(x), x) for x in st))}")
        return bb

    def _handle_blocks(self, handles, fmt: int, flags: int = 0) -> BlockBatch:
        off = torch.tensor([h[0] for h in handles], dtype=torch.int64, device=self.device)
        ln = torch.tensor([h[1] for h in handles], dtype=torch.int64, device=self.device)
        return self._blocks(off, ln, fmt, flags)

    def _raw_kvs(self, handle, columnar: bool) -> dict:
        """The KVs of one metadata block as a host dict: a colblk KeyValueBlock
        (pbl_kv_blocks) or a row block with raw keys."""
        if columnar:
            bb = self._handle_blocks([handle], N.PBL_FMT_ROW)
            kv = kv_blocks(bb)
            st = kv.status()
            if st.any():
                raise DecodeError(f"metadata block corrupt ({N.STATUS_NAMES.get(int(st[0]), st[0])})")
            n = int(kv.blk_base[1].item())
            raw = bb.blocks.cpu().numpy().tobytes()
            ko, kl = kv.key_off[:n].cpu().tolist(), kv.key_len[:n].cpu().tolist()
            vo, vl = kv.val_off[:n].cpu().tolist(), kv.val_len[:n].cpu().tolist()
            return {raw[a:a + m]: raw[c:c + q] for a, m, c, q in zip(ko, kl, vo, vl)}
        from .rowblk import kvs_of_block
        r = decode(self._handle_blocks([handle], N.PBL_FMT_ROW, N.PBL_ROW_RAW_KEYS)).to_host()
        if r["status_mask"]:
            raise DecodeError("metadata block corrupt")
        return {kv.user_key: kv.value for kv in kvs_of_block(r, 0)}

    def metaindex(self) -> dict:
        """Block name -> (offset, length) (decodeColumnarMetaIndex, layout.go:789-824;
        row metaindex before Pebblev6).  The value-block index handle keeps only
        its block handle."""
        if self._meta is None:
            raw = self._raw_kvs(self.footer.metaindex, self.footer.table_format >= N.PBL_TABLE_PEBBLEV6)
            self._meta_raw = raw
            meta = {}
            for k, v in raw.items():
                try:
                    off, i = _uvarint(v)
                    ln, i = _uvarint(v, i)
                except IndexError:
                    raise DecodeError("pebble/table: invalid table (bad block handle)") from None
                if k != VALUE_INDEX_NAME and i != len(v):
                    raise DecodeError("pebble/table: invalid table (bad block handle)")
                meta[k] = (off, ln)
            self._meta = meta
        return self._meta

    def properties(self) -> dict:
        """Property name -> raw value bytes (decodePropertiesBlock, reader.go:601-617)."""
        if self._props is None:
            ph = self.metaindex().get(PROPERTIES_NAME)
            if ph is None and self.footer.table_format == N.PBL_TABLE_LEVELDB:
                self._props = {}  # (LevelDB tables written without one)
                return self._props
            if ph is None:
                raise DecodeError("did not read any value for the properties block in the meta index")
            self._props = self._raw_kvs(ph, self.footer.table_format >= N.PBL_TABLE_PEBBLEV7)
        return self._props

    def index_type(self) -> int:
        v = self.properties().get(INDEX_TYPE_PROP)
        if v is None:
            return 0
        if len(v) < 4:
            raise DecodeError("corrupt index type property")
        return int.from_bytes(v[:4], "little")  # binary.LittleEndian.Uint32 (properties_gen.go:98)

    def two_level(self) -> bool:
        two = self.index_type() == TWO_LEVEL_INDEX
        if self.footer.table_format >= N.PBL_TABLE_PEBBLEV7 and \
                bool(self.footer.attributes & ATTRIBUTE_TWO_LEVEL_INDEX) != two:
            raise DecodeError("pebble/table: attributes mismatch (two-level index)")
        return two

    def key_schema(self) -> int:
        """PBL_FMT_* of the data blocks: rowblk, or the columnar key schema the
        properties name (reader.go:1244-1254: an unknown schema is an error)."""
        if not self.footer.columnar:
            return N.PBL_FMT_ROW
        name = self.properties().get(KEY_SCHEMA_PROP, b"")
        if name == b"crdb1":
            return N.PBL_FMT_COL_CRDB1
        if name.startswith(b"DefaultKeySchema("):
            return N.PBL_FMT_COL_DEFAULT
        raise DecodeError(f"unknown key schema {name!r}")

    def data_block_handles(self) -> IndexHandles:
        """Every data block's handle, in table order, as device arrays."""
        two_level = self.two_level()
        top = self._handle_blocks([self.footer.index], N.PBL_FMT_ROW)
        if self.footer.columnar:
            h = index_handles_col(top)
        else:
            h = index_handles_row(decode(top), 1)
        if h.status().any():
            raise DecodeError("corrupt index block")
        if not two_level:
            return h
        n = h.total(1)
        lower = self._blocks(h.handle_off[:n], h.handle_len[:n], N.PBL_FMT_ROW)
        h2 = index_handles_col(lower) if self.footer.columnar else index_handles_row(decode(lower), lower.n_blocks)
        if h2.status().any():
            raise DecodeError("corrupt lower-level index block")
        return h2

    def data_blocks(self, fmt: Optional[int] = None) -> BlockBatch:
        """The table's data blocks, checksum-verified and decompressed in HBM.
        Row blocks of Pebblev3+ tables carry value prefixes
        (TableFormat.BlockHasValuePrefix; rowblk_iter.go hasValuePrefix)."""
        h = self.data_block_handles()
        n = int(h.blk_base[-1].item())
        fmt = fmt if fmt is not None else self.key_schema()
        flags = N.PBL_ROW_VALUE_PREFIX if (fmt == N.PBL_FMT_ROW and
                                           self.footer.table_format >= N.PBL_TABLE_PEBBLEV1 + 2) else 0
        return self._blocks(h.handle_off[:n], h.handle_len[:n], fmt, flags)

    def value_blocks(self) -> Optional[BlockBatch]:
        """The table's value blocks (metaindex "pebble.value_index": an
        IndexHandle, valblk.go:320-336; its rows through pbl_valblk_index), or
        None when it has none."""
        self.metaindex()
        raw = self._meta_raw.get(VALUE_INDEX_NAME)
        if raw is None:
            return None
        off, i = _uvarint(raw)
        ln, i = _uvarint(raw, i)
        if len(raw) != i + 3:
            raise DecodeError("pebble/table: invalid table (bad value blocks index handle)")
        nw, ow, lw = raw[i], raw[i + 1], raw[i + 2]
        vbi = self._handle_blocks([(off, ln)], N.PBL_FMT_ROW)
        vlen = int(vbi.block_len[0].item())
        rows = vlen // max(1, nw + ow + lw)
        ho = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        hl = torch.empty(max(rows, 1), dtype=torch.int64, device=self.device)
        n_st = torch.zeros(2, dtype=torch.int32, device=self.device)
        src = vbi.blocks.data_ptr() + int(vbi.block_off[0].item())
        rc = N.lib().pbl_valblk_index(src, vlen, nw, ow, lw, ho.data_ptr(), hl.data_ptr(), rows,
                                      n_st.data_ptr(), n_st.data_ptr() + 4, None)
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_valblk_index: {N.STATUS_NAMES.get(rc, rc)}")
        n, st = n_st.cpu().tolist()
        if st != N.PBL_OK:
            raise DecodeError("corrupt value block index")
        return self._blocks(ho[:n], hl[:n], N.PBL_FMT_ROW)

    def decode(self, fmt: Optional[int] = None, resolve: bool = True) -> DecodedBatch:
        """Decode every data block; with `resolve`, values stored in value blocks
        are fetched (pbl_resolve_values) as the table iterator does when it
        returns a value."""
        d = decode(self.data_blocks(fmt))
        if resolve:
            vb = self.value_blocks()
            if vb is not None:
                d = resolve_values(d, vb)
        return d

    def range_dels(self) -> Optional[DecodedBatch]:
        """The table's range-deletion fragments as a run (`pebble_amd.rangedel`):
        the metaindex's "rocksdb.range_del2" block through the physical step and
        the row decode (key = start, trailer = seq << 8 | 15, value = end), or
        None when the table has none.  A columnar table keeps them in a colblk
        keyspan block (colblk/keyspan.go), which `pebble_amd.keyspan.decode`
        turns into the same run."""
        h = self.metaindex().get(RANGE_DEL_NAME)
        if h is None:
            return None
        if self.footer.columnar:
            from .keyspan import decode as keyspan_decode
            d = keyspan_decode(self._handle_blocks([h], N.PBL_FMT_ROW))
            if d.read_totals().status_mask:
                raise DecodeError("range-del keyspan block corrupt "
                                  f"({N.STATUS_NAMES.get(int(d.blk_status[0].item()), '?')})")
            return d
        d = decode(self._handle_blocks([h], N.PBL_FMT_ROW))
        if d.read_totals().status_mask:
            raise DecodeError("range-del block corrupt")
        return d

    def range_keys(self):
        """The table's range-key fragments as a range-key run
        (`pebble_amd.rangekey`): the metaindex's "pebble.range_key" block through
        the physical step and `keyspan.decode(extras=True)` (a `keyspan.Decoded`:
        key = start, value = end, and per KV the suffix and the value), or None
        when the table has none.  A row-format table packs end key, suffixes and
        values into the value (internal/rangekey/rangekey.go); that form is not
        decoded here."""
        h = self.metaindex().get(RANGE_KEY_NAME)
        if h is None:
            return None
        if not self.footer.columnar:
            raise DecodeError("row-format range-key blocks are out of scope: only columnar tables' "
                              "pebble.range_key blocks are read")
        from .keyspan import decode as keyspan_decode
        d = keyspan_decode(self._handle_blocks([h], N.PBL_FMT_ROW), extras=True)
        if d.batch.read_totals().status_mask:
            raise DecodeError("range-key keyspan block corrupt "
                              f"({N.STATUS_NAMES.get(int(d.batch.blk_status[0].item()), '?')})")
        return d

    # -- positioning: batched seeks over the decoded table (pebble_amd.seek) --------
    def comparer(self) -> int:
        """PBL_CMP_* of the table's "rocksdb.comparator" property (the name
        sstable.Reader checks against Options.Comparer, reader.go:1223-1235);
        any other name is an error."""
        name = self.properties().get(COMPARER_PROP, b"")
        if name not in COMPARERS:
            raise DecodeError(f"unknown comparer {name!r}")
        return COMPARERS[name]

    def _seekable(self):
        """The table decoded once, with its fence table."""
        if self._seek is None:
            from .seek import prepare
            comparer = self.comparer()
            d = self.decode(resolve=False)
            if d.read_totals().status_mask:
                raise DecodeError("corrupt data block")
            self._seek = (d, prepare(d, comparer))
        return self._seek

    def _seek_op(self, keys, op: str):
        from .seek import seek
        d, idx = self._seekable()
        return seek(d, keys, op=op, comparer=idx.comparer, index=idx)

    def seek_ge(self, keys):
        """singleLevelIterator.SeekGE of every key: a SeekResult over the KV
        indexes of `decode()`."""
        return self._seek_op(keys, "ge")

    def seek_lt(self, keys):
        return self._seek_op(keys, "lt")

    def get(self, keys, use_filter: bool = False) -> torch.Tensor:
        """Per key, the index of the first KV whose user key equals it
        (PBL_SEEK_EXACT), else -1: int64 [n].  With `use_filter` the table's
        bloom filter is asked first (`seek_prefix_ge`); a bloom filter has no
        false negatives, so the result is the same."""
        r = self.seek_prefix_ge(keys) if use_filter else self.seek_ge(keys)
        return torch.where((r.flags & N.PBL_SEEK_EXACT) != 0, r.kv, torch.full_like(r.kv, -1))

    # -- the table filter (pebble_amd.filter) ----------------------
    def filter(self) -> Optional[torch.Tensor]:
        """The table's bloom filter block as a uint8 device tensor (the
        metaindex's "fullfilter.rocksdb.BuiltinBloomFilter" entry,
        layout.go:1119, through the physical step), or None when the table has
        none.  A table that carries only a filter of another family is a table
        without a filter.  A trailer that does not match the block's length
        raises DecodeError."""
        if self._filter is False:
            from .filter import FILTER_NAME, probe
            h = self.metaindex().get(FILTER_NAME)
            if h is None:
                self._filter = None
                return None
            bb = self._handle_blocks([h], N.PBL_FMT_ROW)
            o, ln = int(bb.block_off[0].item()), int(bb.block_len[0].item())
            f = bb.blocks[o:o + ln]
            if int(probe([f], [b""], N.PBL_CMP_DEFAULT).status[0].item()) != N.PBL_OK:
                raise DecodeError("bloom filter: unexpected cache line size")
            self._filter = f
        return self._filter

    def may_contain(self, keys) -> torch.Tensor:
        """TableFilterDecoder.MayContain of every key's Split-prefix: bool [n],
        all true for a table without a filter."""
        from .filter import probe
        f = self.filter()
        if f is None:
            n = int(keys[1].numel()) - 1 if isinstance(keys, tuple) else len(keys)
            return torch.ones(n, dtype=torch.bool, device=self.device)
        r = probe([f], keys, self.comparer(), device=self.device)
        return (r.may[0] & N.PBL_FILTER_MAY) != 0

    def seek_prefix_ge(self, keys):
        """singleLevelIterator.SeekPrefixGE with the filter block, the prefix
        being each key's own Split-prefix: a SeekResult in which a key the filter
        excludes has kv -1 and PBL_SEEK_FILTERED, and every other key what
        `seek_ge` gives it (one launch, pbl_seek_prefix_batch).  Without a
        filter this is `seek_ge`."""
        f = self.filter()
        if f is None:
            return self.seek_ge(keys)
        from .seek import seek
        d, idx = self._seekable()
        return seek(d, keys, op="ge", comparer=idx.comparer, index=idx, filter=f)

    # -- range scans over the decoded table (pebble_amd.scan) ----------------------
    def _scannable(self, resolve: bool, hide: bool, n: int):
        """The table decoded once per `resolve`, with one ScanIndex per hide flag."""
        from .scan import prepare
        if resolve not in self._scan:
            d = self._seekable()[0] if not resolve else self.decode(resolve=True)
            if d.read_totals().status_mask:
                raise DecodeError("corrupt data block")
            self._scan[resolve] = (d, {})
        d, idx = self._scan[resolve]
        if hide not in idx or idx[hide].n_queries < n:
            idx[hide] = prepare(d, self.comparer(), hide, max(n, 1024))
        return d, idx[hide]

    def scan(self, lowers, uppers, hide_obsolete_points: bool = False, resolve: bool = True):
        """Per range [lower, upper) (None = unbounded), the KVs that
        singleLevelIterator returns for SetBounds(lower, upper); First();
        Next()...: a ScanResult whose batch has one "block" per range and the
        values `decode(resolve=resolve)` holds; `range` and `src_kv` index that
        decode's KVs."""
        from .scan import scan
        d, idx = self._scannable(bool(resolve), bool(hide_obsolete_points), len(lowers))
        return scan(d, lowers, uppers, comparer=idx.comparer, hide_obsolete_points=bool(hide_obsolete_points),
                    index=idx)
