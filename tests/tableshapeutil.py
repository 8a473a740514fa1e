"""The table layer past one pass of every loop and scan: encoders, thresholds, cases.

pebble_amd/csrc/sstable.hip reads index blocks, key-value blocks, the
value-block index and value handles with grid-stride loops and a one-workgroup
scan.  The reference's own tables reach one pass of each.  This file builds
the inputs that reach the next pass, on the test side and from the formats
alone:

  col_index_block   a columnar index block (colblk/index_block.go): separators
                    (RawBytes), offsets (Uint), lengths (Uint), props (RawBytes)
  kv_block          a two-column KeyValueBlock (colblk/key_value_block.go)
  row_index_block   a row index block whose values are block handles
  value_handle      a valblk.Handle behind its prefix byte (valblk.go:190-202)
  valblk_index      the value-block index's fixed-width rows (valblk.go:338-368)
  synthetic_table   a Pebblev7 columnar table on a reference table as template

and the case lists the CPU test (tests/test_table_shapes.py) holds to the
oracle and the GPU test (tests/test_table_shapes_gpu.py) runs.  census() says,
per entry point, which thresholds and encodings the cases cross;
required_census() is what they must cross.  Nothing here calls the device.
"""
import functools
import random

import numpy as np

import oracle
from pebble_amd.colblk import SCHEMA_CRDB1, VALUE_BLOCK_HANDLE, VALUE_IN_PLACE, DataBlockEncoder
from pebble_amd.keyspan import _put_rawbytes, _put_uints
from pebble_amd.rowblk import Writer, make_trailer

# ---- the thresholds, each restating one source line ---------------------------------------
TPB = 256     # common.hip.h:17 kTPB: the write kernels' row stride (sstable.hip:170, 278, 309)
WAVE = 64     # common.hip.h:18 kWave: the wave-per-block kernels' entry stride (sstable.hip:59, 224, 364)
GRID = 4096   # sstable.hip:531, 543-546, 560-564, 590-594 and physical.hip:488-519: the grid cap
SCAN = 1024   # sstable.hip:132-137, 239-245: blocks per chunk of the one-workgroup scans
WAVE_GRID = GRID * TPB // WAVE  # 16384: blocks per pass of a wave-per-block kernel

OK, CORRUPT_BOUNDS, CORRUPT_HEADER, OVERFLOW, CORRUPT_INDEX, CORRUPT_VALUE_HANDLE = 0, 3, 4, 6, 13, 14
DT_UINT, DT_BYTES = 2, 3
U64 = (1 << 64) - 1


def uvarint(x: int, n: int = 0) -> bytes:
    """binary.PutUvarint; with `n`, padded to n bytes by continuation bytes (a
    non-canonical form no writer emits)."""
    out = bytearray()
    while x >= 0x80:
        out.append(x & 0x7F | 0x80)
        x >>= 7
    out.append(x)
    while len(out) < n:
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def varint_len(x: int) -> int:
    return len(uvarint(x))


def pack(blocks, align=8):
    """Blocks back to back, each start `align`-aligned, 16 zero bytes behind the
    last: (buffer, offsets, lengths)."""
    offs, lens, pos = [], [], 0
    for bk in blocks:
        pos = (pos + align - 1) // align * align
        offs.append(pos)
        lens.append(len(bk))
        pos += len(bk)
    buf = np.zeros(pos + 16, np.uint8)
    for o, bk in zip(offs, blocks):
        buf[o:o + len(bk)] = np.frombuffer(bk, np.uint8)
    return buf, np.array(offs, np.uint64), np.array(lens, np.uint32)


# ---- encoders -----------------------------------------------------------------------------------
def _col_block(types, cols, rows: int, force=None, offsets=None) -> bytes:
    """colblk.BlockEncoder without a custom header: version, column count, row
    count, {type, page offset} per column, the pages, one pad byte."""
    force, offsets = force or {}, offsets or {}
    buf = bytearray([1]) + len(types).to_bytes(2, "little") + rows.to_bytes(4, "little")
    hdr = len(buf)
    buf += bytes(5 * len(types))
    for c, (t, data) in enumerate(zip(types, cols)):
        buf[hdr + 5 * c] = t
        buf[hdr + 5 * c + 1:hdr + 5 * c + 5] = len(buf).to_bytes(4, "little")
        if t == DT_BYTES:
            _put_rawbytes(buf, data, force.get(c), offsets.get(c))
        else:
            _put_uints(buf, data, force.get(c))
    buf.append(0)
    return bytes(buf)


def col_index_block(rows, force=None) -> bytes:
    """A columnar index block of rows (separator, offset, length, props).
    `force`: per column index (0 .. 3) the (width, delta) of its Uint encoding
    (the offsets' for a RawBytes column) instead of the smallest one."""
    cols = [[bytes(r[0]) for r in rows], [int(r[1]) for r in rows], [int(r[2]) for r in rows],
            [bytes(r[3]) for r in rows]]
    return _col_block((DT_BYTES, DT_UINT, DT_UINT, DT_BYTES), cols, len(rows), force)


def kv_block(rows, force=None, offsets=None) -> bytes:
    """A KeyValueBlock of rows (key, value).  `offsets`: per column (0, 1) the
    offsets to write instead of the slices' own, for corrupt columns."""
    return _col_block((DT_BYTES, DT_BYTES), [[bytes(r[0]) for r in rows], [bytes(r[1]) for r in rows]], len(rows),
                      force, offsets)


def page_start(block: bytes, col: int) -> int:
    return int.from_bytes(block[7 + 5 * col + 1:7 + 5 * col + 5], "little")


def uint_encoding(block: bytes, col: int) -> str:
    """The Uint encoding byte of column `col`, as colencutil.uint_encoding
    prints it: the width, 'd' appended for a delta base."""
    e = block[page_start(block, col)]
    return f"{e & 0x7f}{'d' if e & 0x80 else ''}"


def handle_value(off: int, length: int, props: bytes = b"") -> bytes:
    return uvarint(off) + uvarint(length) + props


def index_key(i: int) -> bytes:
    """A row index block's key: a separator with its trailer (SeqNumMax, kind 17)."""
    return b"sep%07d" % i + make_trailer((1 << 56) - 1, 17).to_bytes(8, "little")


def row_index_block(entries, restart: int = 1) -> bytes:
    """A row index block of entries (key, value), value = uvarint(offset) ++
    uvarint(length) ++ props (block.HandleWithProperties.EncodeVarints) -- or
    any other bytes, for the corrupt ones."""
    w = Writer(restart)
    for k, v in entries:
        w.add_raw(k, v)
    return w.finish()


def value_handle(vlen: int, block_num: int, off: int, prefix: int = 0x80) -> bytes:
    """Prefix byte, then uvarint ValueLen, BlockNum, OffsetInBlock."""
    return bytes([prefix]) + uvarint(vlen) + uvarint(block_num) + uvarint(off)


def ref_decode_handle(src: bytes):
    """valblk.DecodeHandle (valblk.go:206-279) restated: (ValueLen, BlockNum,
    OffsetInBlock), each a varint of at most five bytes read into 32 bits, the
    fifth byte taken whole, without a look at its continuation bit."""
    out, p = [], 0
    for _ in range(3):
        v = 0
        for i in range(5):
            b = src[p]
            p += 1
            if i == 4 or b < 128:
                v |= b << (7 * i)
                break
            v |= (b & 0x7F) << (7 * i)
        out.append(v & 0xFFFFFFFF)
    return tuple(out)


def valblk_index(handles, widths, nums=None) -> bytes:
    """valblk index rows: block number, offset, length, little-endian at
    `widths` = (num, off, len) bytes; `nums` replaces the block numbers."""
    nw, ow, lw = widths
    out = bytearray()
    for i, (o, ln) in enumerate(handles):
        n = i if nums is None else nums[i]
        out += n.to_bytes(nw, "little") + o.to_bytes(ow, "little") + ln.to_bytes(lw, "little")
    return bytes(out)


def decode_valblk_index(data: bytes, widths):
    """valblk.DecodeIndex (valblk.go:340-368) restated: (handles, error).  The
    reference does not look at the widths themselves; the writer emits 1..8
    (littleEndianPut), which is all this restatement takes."""
    nw, ow, lw = widths
    assert all(1 <= w <= 8 for w in widths)
    out, i, w = [], 0, nw + ow + lw
    while data:
        if len(data) < w:
            return None, "does not contain a full entry"
        if int.from_bytes(data[:nw], "little") != i:
            return None, "unexpected block num"
        i += 1
        out.append((int.from_bytes(data[nw:nw + ow], "little"), int.from_bytes(data[nw + ow:w], "little")))
        data = data[w:]
    return out, None


def corrupt_row_block() -> bytes:
    """A row block whose restart count is 0: the row decode's
    PBL_CORRUPT_NO_RESTARTS (rowblk_iter.go: "invalid table (block has no restart points)")."""
    w = Writer(1)
    w.add_raw(index_key(0), handle_value(1, 2))
    b = bytearray(w.finish())
    b[-4:] = bytes(4)
    return bytes(b)


# ---- pbl_index_handles_col ----------------------------------------------------------------------
UINT_FORMS = ("0", "0d", "1", "2", "4", "8", "1d", "2d", "4d")  # every UintEncoding IsValid accepts
BIG = (1 << 33) + 5  # a delta base above 2^32


def _form_values(form: str, n: int, rng: random.Random):
    """n values that the Uint encoding `form` holds, and its (width, delta)."""
    w, delta = int(form.rstrip("d")), form.endswith("d")
    base = BIG if delta else 0
    if w == 0:
        return [base] * n, (0, delta)
    top = (1 << 8 * w) - 1
    vals = [base, base + top] + [base + rng.randint(0, top) for _ in range(n - 2)]
    return vals, (w, delta)


def _sep(i: int) -> bytes:
    return b"s%06d" % i


@functools.lru_cache(maxsize=None)
def index_col_shape_cases():
    """(name, block, rows it was built from): the row counts, every Uint form
    of offsets and lengths, the props' offset widths."""
    rng = random.Random(71)
    out = []
    for n in (0, 1, 255, 256, 257, 1000):
        rows = [(_sep(i), 1000 * i + 7, 100 + i % 50, b"p%d" % (i % 7) if i % 3 else b"") for i in range(n)]
        out.append((f"rows{n}", col_index_block(rows), rows))
    for k, fo in enumerate(UINT_FORMS):
        fl = UINT_FORMS[(k + 4) % len(UINT_FORMS)]
        n = 9 + k
        offs, eo = _form_values(fo, n, rng)
        lens, el = _form_values(fl, n, rng)
        rows = [(_sep(i), offs[i], lens[i], b"x" * (i % 4)) for i in range(n)]
        out.append((f"off{fo}_len{fl}", col_index_block(rows, force={1: eo, 2: el}), rows))
    # the encodings a writer picks on its own: offsets past 64 KiB and 4 GiB, all lengths equal
    for name, step in (("file64k", 9000), ("file4g", 600_000_000)):
        rows = [(_sep(i), step * i, 4091, b"") for i in range(12)]
        out.append((name, col_index_block(rows), rows))
    # props: all empty (constant offsets), > 255 bytes (2-byte offsets), > 65535 bytes (4-byte offsets)
    for name, n, plen in (("props_empty", 20, 0), ("props300", 30, 10), ("props70000", 1000, 70)):
        rows = [(_sep(i), 50 * i, 45, bytes([65 + i % 26]) * plen) for i in range(n)]
        out.append((name, col_index_block(rows), rows))
    return tuple(out)


def _tiny_index_rows(i: int):
    return [(_sep(3 * i + j), 40_000 * i + 13_000 * j, 12_000 + (i + j) % 900, b"q" * ((i + j) % 3))
            for j in range(i % 3 + 1)]


@functools.lru_cache(maxsize=None)
def index_col_pool():
    """GRID + 1 index blocks of 1 .. 3 rows: (blocks, their rows).  The batches
    are its prefixes."""
    rows = [_tiny_index_rows(i) for i in range(GRID + 1)]
    return tuple(col_index_block(r) for r in rows), tuple(rows)


INDEX_COL_BATCHES = (1, SCAN - 1, SCAN, SCAN + 1, GRID + 1)


@functools.lru_cache(maxsize=None)
def index_col_malformed():
    """(name, block): wrong column type, 3 columns, row counts the pages cannot
    hold, every proper prefix of a small valid block.  The status is the
    oracle's to say."""
    rows = [(_sep(i), 100 * i, 90, b"ab" * (i % 2)) for i in range(5)]
    good = col_index_block(rows)
    out = []
    for col in range(4):
        b = bytearray(good)
        b[7 + 5 * col] = DT_UINT if b[7 + 5 * col] == DT_BYTES else DT_BYTES
        out.append((f"type_col{col}", bytes(b)))
    b = bytearray(good)
    b[1:3] = (3).to_bytes(2, "little")
    out.append(("three_columns", bytes(b)))
    for n in (6, 10, 300):
        out.append((f"rows{n}_of5", good[:3] + n.to_bytes(4, "little") + good[7:]))
    out += [(f"prefix{n}", good[:n]) for n in range(len(good))]
    return good, tuple(out)


# ---- pbl_index_handles_row ----------------------------------------------------------------------
def _varint_value(n: int) -> int:
    """The largest value whose uvarint takes n bytes."""
    return min((1 << 7 * n) - 1, U64)


def _row_entry(i: int):
    """Entry i: offset and length varints of every length 1 .. 10, out of step."""
    a, b = i % 10 + 1, (i // 10 + i) % 10 + 1
    off = _varint_value(a) - (i % 3 if a > 1 else 0)
    ln = _varint_value(b) - (i % 2 if b > 1 else 0)
    return off, ln, b"pr" * (i % 3)


@functools.lru_cache(maxsize=None)
def index_row_shape_cases():
    """(name, block, [(off, len, props)]): 1, 63, 64, 65 and 300 entries."""
    out = []
    for n, restart in ((1, 1), (63, 1), (64, 16), (65, 1), (300, 16), (100, 1)):
        ents = [_row_entry(i) for i in range(n)]
        out.append((f"entries{n}", row_index_block([(index_key(i), handle_value(*e)) for i, e in enumerate(ents)],
                                                   restart), ents))
    return tuple(out)


BAD_VARINTS = {"tenth_byte": b"\xff" * 9 + b"\x02", "unterminated": b"\x80"}


@functools.lru_cache(maxsize=None)
def index_row_corrupt_cases():
    """(name, block): a tenth byte above 1 and an unterminated varint, in the
    offset and in the length, in entry 0, in entry 70 and in the last entry of
    100."""
    out = []
    for kind, bad in BAD_VARINTS.items():
        for field in ("off", "len"):
            for at in (0, 70, 99):
                ents = []
                for i in range(100):
                    v = handle_value(*_row_entry(i))
                    if i == at:
                        v = bad if field == "off" else uvarint(5) + bad
                    ents.append((index_key(i), v))
                out.append((f"{kind}_{field}_entry{at}", row_index_block(ents)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def index_row_pool():
    """WAVE_GRID + 1 one-entry blocks: (blocks, [(off, len, props)])."""
    ents = [_row_entry(i) for i in range(WAVE_GRID + 1)]
    w = Writer(1)
    blocks = []
    for i, e in enumerate(ents):
        w.reset(1)
        w.add_raw(index_key(i), handle_value(*e))
        blocks.append(w.finish())
    return tuple(blocks), tuple(ents)


# ---- pbl_kv_blocks -------------------------------------------------------------------------------
KV_ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
KV_BATCHES = (SCAN + 1, GRID + 1, WAVE_GRID + 1)


@functools.lru_cache(maxsize=None)
def kv_shape_cases():
    """(name, block, rows): the row counts with empty keys and values among
    them, offsets of 1, 2 and 4 bytes, all keys / all values empty (constant
    offsets)."""
    out = []
    for n in KV_ROWS:
        rows = [(b"k%04d" % i if i % 5 else b"", b"v" * (i % 4)) for i in range(n)]
        out.append((f"rows{n}", kv_block(rows), rows))
    rows = [(b"key%03d" % i, bytes([i]) * 20) for i in range(40)]      # values 800 bytes: 2-byte offsets
    out.append(("off2", kv_block(rows), rows))
    rows = [(b"k%d" % i, bytes([97 + i]) * 7000) for i in range(10)]   # values 70000 bytes: 4-byte offsets
    out.append(("off4", kv_block(rows), rows))
    rows = [(b"", b"value%d" % i) for i in range(9)]
    out.append(("keys_empty", kv_block(rows), rows))
    rows = [(b"key%d" % i, b"") for i in range(9)]
    out.append(("values_empty", kv_block(rows), rows))
    rows = [(b"wide%d" % i, b"w" * i) for i in range(9)]
    out.append(("forced_off4", kv_block(rows, force={0: (4, False), 1: (2, False)}), rows))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kv_pool():
    rows = [[(b"name%05d" % i, uvarint(i * 37) + uvarint(i % 900))] + [(b"x", b"")] * (i % 2)
            for i in range(WAVE_GRID + 1)]
    return tuple(kv_block(r) for r in rows), tuple(rows)


@functools.lru_cache(maxsize=None)
def kv_corrupt_cases():
    """(name, block): offsets that decrease (in row 0, in a row >= 64, in the
    last row, of keys and of values) and a last offset past the block."""
    rows = [(b"k%03d" % i, b"val%03d" % i) for i in range(100)]
    ends = {0: [4 * i for i in range(101)], 1: [6 * i for i in range(101)]}
    out = []
    for col in (0, 1):
        for at in (0, 70, 99):
            offs = list(ends[col])
            if at == 0:
                offs[0], offs[1] = 3, 2
            elif at == 99:
                offs[99] = offs[100] + 1  # (the last offset stays the data's length: Init accepts the column)
            else:
                offs[at + 1] = offs[at] - 1
            out.append((f"decreasing_col{col}_row{at}", kv_block(rows, offsets={col: offs})))
        offs = list(ends[col])
        offs[-1] += 4000
        out.append((f"last_past_block_col{col}", kv_block(rows, offsets={col: offs})))
    return tuple(out)


# ---- pbl_valblk_index ----------------------------------------------------------------------------
VALBLK_ROWS = (0, 1, 255, 256, 257, 1000)
VALBLK_WIDTHS = ((1, 1, 1), (2, 3, 2), (3, 5, 3), (2, 8, 4), (4, 4, 4), (5, 6, 7), (8, 8, 8), (2, 7, 1))


def valblk_handles(n: int, widths):
    _nw, ow, lw = widths
    return [((i * 0x9E3779B97F4A7C15) & ((1 << 8 * ow) - 1), (i * 0xC2B2AE3D27D4EB4F + 1) & ((1 << 8 * lw) - 1))
            for i in range(n)]


@functools.lru_cache(maxsize=None)
def valblk_cases():
    """(name, bytes, widths): every width triple at a row count it can number,
    every row count; wrong block numbers; a ragged length."""
    out = []
    for k, w in enumerate(VALBLK_WIDTHS):
        n = VALBLK_ROWS[(k + 2) % len(VALBLK_ROWS)]
        assert n <= 1 << 8 * w[0]
        out.append((f"w{w}_rows{n}", valblk_index(valblk_handles(n, w), w), w))
    for n in VALBLK_ROWS:
        w = (2, 3, 2)
        out.append((f"rows{n}", valblk_index(valblk_handles(n, w), w), w))
    w = (2, 3, 2)
    for at in (0, 256, 299):
        nums = list(range(300))
        nums[at] += 1
        out.append((f"wrong_num_row{at}", valblk_index(valblk_handles(300, w), w, nums), w))
    out.append(("ragged", valblk_index(valblk_handles(300, w), w)[:-3], w))
    return tuple(out)


# ---- pbl_resolve_values --------------------------------------------------------------------------
N_VALUE_BLOCKS = 131
BIG_VALUE = 16400  # > 16383: a 3-byte ValueLen


@functools.lru_cache(maxsize=None)
def value_blocks():
    """131 value blocks: block 0 of 20000 bytes (offsets of 3 varint bytes),
    the others of 40 .. 300."""
    rng = random.Random(5)
    return tuple(rng.randbytes(20000 if i == 0 else 40 + (i * 53) % 261) for i in range(N_VALUE_BLOCKS))


def crdb_key(i: int, wall: int = 1_700_000_000_000_000_000) -> bytes:
    return b"k%07d" % i + b"\x00" + (wall + i).to_bytes(8, "big") + b"\x09"


def _handle_for(i: int, vbs):
    """The i-th handle of the shape cases: (vlen, block, offset), walking the
    varint lengths of all three fields."""
    pick = (i // 4 + 3 * (i % 4)) % 8  # (i % 4 == 1 is an in-place value: i // 4 walks every pick)
    if pick == 0:
        return (BIG_VALUE if i % 1024 == 0 else 200 + i % 100, 0, 100 + i % 50)  # ValueLen 3 / 2 bytes
    if pick == 1:
        return (130 + i % 60, 0, 16384 + i % 3000)                              # offset 3 bytes
    if pick == 2:
        bn = 128 + i % (len(vbs) - 128)                                         # block number 2 bytes
        return (len(vbs[bn]) - 5, bn, 5)                                        # ends at its block's end
    bn = 1 + i % 127
    n = len(vbs[bn])
    if pick == 3:
        return (0, bn, 0)
    if pick == 4:
        return (0, bn, n)                                                       # empty, at offset == block length
    if pick == 5:
        return (n - 128 if n > 140 else 3, bn, 128 if n > 140 else 0)           # offset 2 bytes
    return (1 + i % 30, bn, i % 8)


def resolve_kvs(first: int, n: int, vbs):
    """n KVs (key number, in-place value or None, handle or None, expected
    value): three in four values are handles."""
    out = []
    for i in range(first, first + n):
        if i % 4 == 1:
            v = b"inplace%d" % i if i % 8 else b""
            out.append((i, v, None, v))
        else:
            vlen, bn, off = _handle_for(i, vbs)
            out.append((i, None, (vlen, bn, off), vbs[bn][off:off + vlen]))
    return out


def row_data_block(kvs, restart: int = 16, raw_handles=None) -> bytes:
    """A row data block with value prefixes (Pebblev3+): SET KVs whose value is
    in place (prefix 0x00) or a value-block handle (prefix 0x80).
    `raw_handles`: {key number: the bytes behind the prefix byte}, for corrupt handles."""
    w = Writer(restart)
    for i, v, h, _e in kvs:
        k = b"k%07d" % i
        if raw_handles and i in raw_handles:
            w.add_with_optional_value_prefix(k, make_trailer(i + 1, 1), False, raw_handles[i], len(k), True, 0x80, False)
        elif h is None:
            w.add_with_optional_value_prefix(k, make_trailer(i + 1, 1), False, v, len(k), True, 0x00, False)
        else:
            w.add_with_optional_value_prefix(k, make_trailer(i + 1, 1), False, value_handle(*h)[1:], len(k), True,
                                             0x80, False)
    return w.finish()


def col_data_block(kvs, raw_handles=None) -> bytes:
    """A crdb1 colblk data block of the same KVs."""
    w = DataBlockEncoder(SCHEMA_CRDB1)
    for i, v, h, _e in kvs:
        if raw_handles and i in raw_handles:
            w.add(crdb_key(i), make_trailer(i + 1, 1), raw_handles[i], VALUE_BLOCK_HANDLE)
        elif h is None:
            w.add(crdb_key(i), make_trailer(i + 1, 1), v, VALUE_IN_PLACE)
        else:
            w.add(crdb_key(i), make_trailer(i + 1, 1), value_handle(*h)[1:], VALUE_BLOCK_HANDLE)
    return w.finish()


RESOLVE_KVS = (1, 63, 64, 65, 200)
RESOLVE_BATCHES = (SCAN + 1, GRID + 1, WAVE_GRID + 1)


@functools.lru_cache(maxsize=None)
def resolve_shape_cases():
    """(row blocks, colblk blocks, kvs per block): blocks of 1, 63, 64, 65 and
    200 KVs, in-place and handle values mixed."""
    vbs = value_blocks()
    kvs, first = [], 0
    for n in RESOLVE_KVS:
        kvs.append(resolve_kvs(first, n, vbs))
        first += n
    return tuple(row_data_block(k) for k in kvs), tuple(col_data_block(k) for k in kvs), tuple(kvs)


@functools.lru_cache(maxsize=None)
def resolve_pool(fmt: str):
    """WAVE_GRID + 1 blocks of 1 .. 3 KVs over the shared value blocks:
    (blocks, kvs per block); `fmt`: "row" or "col"."""
    vbs = value_blocks()
    kvs, first = [], 0
    for b in range(WAVE_GRID + 1):
        n = b % 3 + 1
        kvs.append(resolve_kvs(first, n, vbs))
        first += n
    build = row_data_block if fmt == "row" else col_data_block
    return tuple(build(k) for k in kvs), tuple(kvs)


@functools.lru_cache(maxsize=None)
def resolve_corrupt_cases():
    """(name, bytes behind the prefix byte, expected value or None = corrupt):
    the edges of valueBlockFetcher's bounds and of the handle's own length."""
    vbs = value_blocks()
    n7 = len(vbs[7])
    h = value_handle(300, 0, 16500)[1:]
    a, c = varint_len(300), varint_len(0)
    return (
        ("ends_at_block_end", value_handle(n7 - 3, 7, 3)[1:], vbs[7][3:]),
        ("one_byte_longer", value_handle(n7 - 2, 7, 3)[1:], None),
        ("offset_past_block", value_handle(0, 7, n7 + 1)[1:], None),
        ("block_num_is_n_blocks", value_handle(1, len(vbs), 0)[1:], None),
        ("cut_after_len", h[:a], None),
        ("cut_after_block_num", h[:a + c], None),
        ("cut_inside_offset", h[:-1], None),
        ("prefix_byte_alone", b"", None),
        ("value_len_2_32", value_handle(1 << 32, 0, 0)[1:], None),
        # the varint divergence: the reference reads at most five
        # bytes per field, unchecked; the device reads Go's 64-bit Uvarint
        ("six_byte_len_padded", uvarint(5, 6) + uvarint(7) + uvarint(0), vbs[7][:5]),
        ("six_byte_block_num_padded", uvarint(5) + uvarint(7, 6) + uvarint(0), vbs[7][:5]),
        ("eleven_byte_len", b"\x80" * 10 + b"\x01" + uvarint(7) + uvarint(0), None),
        ("tenth_byte_2", b"\xff" * 9 + b"\x02" + uvarint(7) + uvarint(0), None),
    )


@functools.lru_cache(maxsize=None)
def resolve_corrupt_batch(fmt: str):
    """(blocks, kvs per block, expected status per block): a good block, one
    block of three KVs per corrupt case with the case in the middle, a good
    block; the row batch also holds a block the row decode rejects."""
    vbs = value_blocks()
    build = row_data_block if fmt == "row" else col_data_block
    good = resolve_kvs(0, 3, vbs)
    blocks, kvs, st = [build(good)], [good], [OK]
    for c, (_name, raw, exp) in enumerate(resolve_corrupt_cases()):
        ks = resolve_kvs(10 * (c + 1), 3, vbs)
        i = ks[1][0]
        ks[1] = (i, None, None, exp)
        blocks.append(build(ks, raw_handles={i: raw}))
        kvs.append(ks)
        st.append(OK if exp is not None else CORRUPT_VALUE_HANDLE)
        if fmt == "row" and c == 4:
            blocks.append(corrupt_row_block())
            kvs.append([])
            st.append(1)  # PBL_CORRUPT_NO_RESTARTS
    last = resolve_kvs(1000, 5, vbs)
    return tuple(blocks + [build(last)]), tuple(kvs + [last]), tuple(st + [OK])


ALIAS_VALUE = (4096, 0, 1000)  # 300 handles name these 4 KiB of value block 0
ALIAS_HANDLES = 300


@functools.lru_cache(maxsize=None)
def resolve_alias_case():
    """(blocks, kvs per block): 300 handles naming the same 4 KiB, ten to a
    block, so the resolved bytes pass the input bytes many times over."""
    vbs = value_blocks()
    vlen, bn, off = ALIAS_VALUE
    kvs = [[(10 * b + j, None, ALIAS_VALUE, vbs[bn][off:off + vlen]) for j in range(10)]
           for b in range(ALIAS_HANDLES // 10)]
    return tuple(row_data_block(k) for k in kvs), tuple(kvs)


# ---- the whole table -----------------------------------------------------------------------------
TABLE_DATA_BLOCKS = GRID + 4      # 4100
TABLE_PER_INDEX = 4               # 1025 lower-level index blocks: the top level has 1025 rows
VALUE_INDEX_WIDTHS = (1, 3, 2)


def _table_kvs(vbs):
    """Per data block its (key, trailer, value kind, stored value, resolved value)."""
    out, i = [], 0
    for b in range(TABLE_DATA_BLOCKS):
        blk = []
        for _ in range(b % 3 + 1):
            if i % 3 == 0:
                bn = (i // 3) % len(vbs)
                n = len(vbs[bn])
                if i == 0:
                    h = (BIG_VALUE, 0, 3000)
                elif bn == 0:
                    h = (150 + i % 50, 0, 16384 + i % 3000)
                else:
                    off = i % 7
                    h = (n - off if i % 2 else min(n - off, 1 + i % 40), bn, off)
                blk.append((crdb_key(i), make_trailer(i + 1, 1), VALUE_BLOCK_HANDLE, value_handle(*h)[1:],
                            vbs[h[1]][h[2]:h[2] + h[0]]))
            else:
                v = b"value-of-%d" % i if i % 5 else b""
                blk.append((crdb_key(i), make_trailer(i + 1, 1), VALUE_IN_PLACE, v, v))
            i += 1
        out.append(blk)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_table(template: bytes):
    """A Pebblev7 columnar (crdb1) table in `template`'s format, whose
    properties block, footer layout and attributes are reused: TABLE_DATA_BLOCKS
    data blocks of 1 .. 3 KVs, a two-level index with four data blocks per
    lower-level block, the 131 value blocks behind a value-block index of
    widths (1, 3, 2), a metaindex naming the properties and the value index, and
    the footer with its checksum recomputed.  Returns (table bytes, info) with
    info = dict(kvs=[(user key, trailer, resolved value)], stored=[(stored
    value, is handle)], data_handles=[(offset, length)], lower=…, n_value_blocks)."""
    f = oracle.parse_footer(template[-61:], len(template))
    assert f is not None and f["table_format"] == 9 and f["footer"][1] == 61 and f["attributes"] & (1 << 5)
    ck = f["checksum_type"]
    st, meta = oracle.kv_block_col(oracle.table_block(template, f["metaindex"], ck))
    assert st == 0
    props = oracle.table_block(template, oracle.decode_handle(dict(meta)[b"rocksdb.properties"], 0)[0], ck)
    vbs = value_blocks()
    body = bytearray()

    def put(block: bytes):
        off = len(body)
        body.extend(block + b"\0")
        body.extend(oracle.block_checksum(ck, block + b"\0").to_bytes(4, "little"))
        return off, len(block)

    data_handles, lower_rows, kvs, stored = [], [], [], []
    for blk in _table_kvs(vbs):
        w = DataBlockEncoder(SCHEMA_CRDB1)
        for k, t, kind, sv, rv in blk:
            w.add(k, t, sv, kind)
            kvs.append((k, t, rv))
            stored.append((sv, kind == VALUE_BLOCK_HANDLE))
        h = put(w.finish())
        data_handles.append(h)
        lower_rows.append((blk[-1][0], h[0], h[1], b""))
    vb_handles = [put(v) for v in vbs]
    top_rows, lower_handles = [], []
    for i in range(0, len(lower_rows), TABLE_PER_INDEX):
        rows = lower_rows[i:i + TABLE_PER_INDEX]
        h = put(col_index_block(rows))
        lower_handles.append(h)
        top_rows.append((rows[-1][0], h[0], h[1], b""))
    vih = put(valblk_index(vb_handles, VALUE_INDEX_WIDTHS))
    ih = put(col_index_block(top_rows))
    ph = put(props)
    mh = put(kv_block([(b"pebble.value_index", uvarint(vih[0]) + uvarint(vih[1]) + bytes(VALUE_INDEX_WIDTHS)),
                       (b"rocksdb.properties", uvarint(ph[0]) + uvarint(ph[1]))]))
    foot = bytearray(template[f["footer"][0]:f["footer"][0] + 61])
    foot[1:41] = (uvarint(mh[0]) + uvarint(mh[1]) + uvarint(ih[0]) + uvarint(ih[1])).ljust(40, b"\0")
    foot[45:49] = oracle.crc32c(bytes(foot[:45] + foot[49:])).to_bytes(4, "little")
    info = dict(kvs=kvs, stored=stored, data_handles=data_handles, lower=lower_handles,
                n_value_blocks=len(vbs), top_rows=len(top_rows))
    return bytes(body) + bytes(foot), info


# ---- physical.hip ---------------------------------------------------------------------------------
PHYS_CHECKSUM_BLOCKS = WAVE_GRID + 1
PHYS_DECOMPRESS_BLOCKS = GRID + 1
CORRUPT_EVERY = 1000


@functools.lru_cache(maxsize=None)
def checksum_batch(kind: int):
    """WAVE_GRID + 1 physical blocks of 0 .. 8 bytes (block, indicator byte 0,
    checksum), every 1000th with a wrong stored checksum: (file bytes, offsets,
    lengths, expected computed checksums, expected statuses)."""
    rng = random.Random(kind)
    body, offs, lens, comp, st = bytearray(), [], [], [], []
    for i in range(PHYS_CHECKSUM_BLOCKS):
        blk = rng.randbytes(i % 9)
        c = oracle.block_checksum(kind, blk + b"\0")
        bad = i % CORRUPT_EVERY == CORRUPT_EVERY - 1
        offs.append(len(body))
        lens.append(len(blk))
        comp.append(c)
        st.append(10 if bad else 0)
        body += blk + b"\0" + ((c ^ (1 << (i % 32))) if bad else c).to_bytes(4, "little")
    return bytes(body), np.array(offs, np.uint64), np.array(lens, np.uint32), np.array(comp, np.uint32), \
        np.array(st, np.uint32)


@functools.lru_cache(maxsize=None)
def decompress_batch():
    """GRID + 1 tiny physical blocks, stored and snappy by turns: (file bytes,
    offsets, lengths, expected decoded blocks from the oracle)."""
    from snappyutil import assemble, c1, lit
    rng = random.Random(11)
    body, offs, lens, exp = bytearray(), [], [], []
    for i in range(PHYS_DECOMPRESS_BLOCKS):
        raw = rng.randbytes(1 + i % 13)
        if i % 2:
            blk, _ = assemble([lit(raw)] + ([c1(len(raw), 4 + i % 8)] if len(raw) >= 4 and i % 4 == 1 else []))
            want = oracle.snappy_decode(blk)
            ind = 1
        else:
            blk, want, ind = raw, raw, 0
        assert want is not None
        offs.append(len(body))
        lens.append(len(blk))
        exp.append(want)
        body += blk + bytes([ind]) + bytes(4)
    return bytes(body), np.array(offs, np.uint64), np.array(lens, np.uint32), tuple(exp)


# ---- the census ------------------------------------------------------------------------------------
def _block_crossings(counts) -> set:
    out = set()
    for n in counts:
        out |= {name for name, t in (("blocks>SCAN", SCAN), ("blocks>GRID", GRID), ("blocks>WAVE_GRID", WAVE_GRID))
                if n > t}
    return out


def _side(n: int, t: int, what: str) -> str:
    return f"{what}{'>' if n > t else '<='}{'TPB' if t == TPB else 'WAVE'}"


def census() -> dict:
    """Per entry point, the crossings its cases hold, read from the cases (and
    for encodings from the blocks' own bytes)."""
    c = {}
    # pbl_index_handles_col
    s = set()
    for _name, blk, rows in index_col_shape_cases():
        s.add(_side(len(rows), TPB, "rows"))
        if rows:
            s |= {("offsets", uint_encoding(blk, 1)), ("lengths", uint_encoding(blk, 2)),
                  ("props_offsets", uint_encoding(blk, 3))}
    s |= _block_crossings(INDEX_COL_BATCHES)
    _buf, off, _lens = pack(index_col_pool()[0], 1)
    s |= {("residue", int(r)) for r in set((off % 8).tolist())}
    c["pbl_index_handles_col"] = s
    # pbl_index_handles_row
    s = set()
    for _name, _blk, ents in index_row_shape_cases():
        s.add(_side(len(ents), WAVE, "entries"))
        for o, ln, _p in ents:
            s |= {("offset_varint", varint_len(o)), ("length_varint", varint_len(ln))}
    s |= _block_crossings([len(index_row_pool()[0])])
    c["pbl_index_handles_row"] = s
    # pbl_kv_blocks
    s = set()
    for _name, blk, rows in kv_shape_cases():
        s |= {_side(len(rows), TPB, "rows"), _side(len(rows), WAVE, "entries")}
        if rows:
            s |= {("key_offsets", uint_encoding(blk, 0)), ("value_offsets", uint_encoding(blk, 1))}
    s |= _block_crossings(KV_BATCHES)
    c["pbl_kv_blocks"] = s
    # pbl_valblk_index
    s = set()
    for _name, data, w in valblk_cases():
        s.add(_side(len(data) // sum(w), TPB, "rows"))
        s.add(("widths", w))
    c["pbl_valblk_index"] = s
    # pbl_resolve_values
    s = set()
    pools = [k for blk in resolve_pool("row")[1] for k in blk]
    for kvs in resolve_shape_cases()[2]:
        s.add(_side(len(kvs), WAVE, "entries"))
        pools += kvs
    for _i, _v, h, _e in pools:
        if h is not None:
            s |= {("value_len_varint", varint_len(h[0])), ("block_num_varint", varint_len(h[1])),
                  ("offset_varint", varint_len(h[2]))}
    s |= _block_crossings(RESOLVE_BATCHES)
    s.add(("value_blocks>129", len(value_blocks()) > 129))
    c["pbl_resolve_values"] = s
    c["pbl_verify_checksums"] = _block_crossings([PHYS_CHECKSUM_BLOCKS])
    c["pbl_decompress_blocks"] = _block_crossings([PHYS_DECOMPRESS_BLOCKS])
    return c


def required_census() -> dict:
    """What the cases must hold -- no more, no fewer."""
    rows = {"rows<=TPB", "rows>TPB"}
    ents = {"entries<=WAVE", "entries>WAVE"}
    forms = set(UINT_FORMS)
    return {
        "pbl_index_handles_col": rows | {"blocks>SCAN", "blocks>GRID"}
        | {(col, f) for col in ("offsets", "lengths") for f in forms}
        | {("props_offsets", f) for f in ("0", "1", "2", "4")} | {("residue", r) for r in range(8)},
        "pbl_index_handles_row": ents | {"blocks>SCAN", "blocks>GRID", "blocks>WAVE_GRID"}
        | {(f, n) for f in ("offset_varint", "length_varint") for n in range(1, 11)},
        "pbl_kv_blocks": rows | ents | {"blocks>SCAN", "blocks>GRID", "blocks>WAVE_GRID"}
        | {(col, f) for col in ("key_offsets", "value_offsets") for f in ("0", "1", "2", "4")},
        "pbl_valblk_index": rows | {("widths", w) for w in VALBLK_WIDTHS},
        "pbl_resolve_values": ents | {"blocks>SCAN", "blocks>GRID", "blocks>WAVE_GRID", ("value_blocks>129", True)}
        | {("value_len_varint", n) for n in (1, 2, 3)} | {("block_num_varint", n) for n in (1, 2)}
        | {("offset_varint", n) for n in (1, 2, 3)},
        "pbl_verify_checksums": {"blocks>SCAN", "blocks>GRID", "blocks>WAVE_GRID"},
        "pbl_decompress_blocks": {"blocks>SCAN", "blocks>GRID"},
    }
