"""Directed colblk blocks: every column encoding in every region of the decode.

The device decode reads each column through one function (u_at / Src::le / g_le,
pebble_amd/csrc/colblk_block.hip.h) whose path depends on the column's Uint
width and delta bit, on where the byte lies (staged head, staged tail, global
memory) and on the block's alignment.  The random blocks of colutil.py reach a
small part of that space; the matrix below reaches all of it on purpose:

  describe       the encodings a block holds, read from its bytes alone (the
                 layout of colutil.py: custom header, version, column count,
                 rows, {type, page offset} per column); no decoder involved
  directed_rows  rows (colutil.random_rows' tuple shape) whose knobs force each
                 column's encoding independently
  matrix         the blocks, built once; tests/test_colblk_encodings.py asserts
                 the exact set of cells they cover, tests/test_colblk_encodings_gpu.py
                 decodes them on every route

The expected decode of every block is colutil.build_block's: derived from the
writer's input (expected_key), never from a decoder.
"""
import functools
import random
import struct
from dataclasses import dataclass, field

from colutil import build_block, build_block_meta
from pebble_amd.colblk import (SCHEMA_CRDB1, SCHEMA_DEFAULT, VALUE_BLOB_HANDLE, VALUE_BLOCK_HANDLE,
                               VALUE_IN_PLACE)

# ---- the header reader ---------------------------------------------------------------
DT_BOOL, DT_UINT, DT_BYTES, DT_PREFIX = 1, 2, 3, 4
COLUMNS = {
    SCHEMA_DEFAULT: ["prefix", "suffix", "trailers", "prefix_changed", "values", "external", "obsolete"],
    SCHEMA_CRDB1: ["prefix", "wall", "logical", "untyped", "trailers", "prefix_changed", "values", "external",
                   "obsolete"],
}
TIERING_COLUMNS = ["span", "attr", "handles"]
SCHEMA_NAME = {SCHEMA_DEFAULT: "default", SCHEMA_CRDB1: "crdb1"}


def custom_header(schema: int) -> int:
    """Bytes before the block header: the maximum key length (LE32), after the
    crdb1 schema's suffix-types byte."""
    return 5 if schema == SCHEMA_CRDB1 else 4


def column_names(schema: int, tiering: bool = False) -> list:
    return COLUMNS[schema] + (TIERING_COLUMNS if tiering else [])


def column_pages(block: bytes, schema: int, tiering: bool = False) -> dict:
    """{column name: (data type, page start)} from the block's column directory."""
    c0 = custom_header(schema)
    names = column_names(schema, tiering)
    assert block[c0] == 1, "colblk version"
    assert int.from_bytes(block[c0 + 1:c0 + 3], "little") == len(names), "column count"
    out = {}
    for i, name in enumerate(names):
        h = c0 + 7 + 5 * i
        out[name] = (block[h], int.from_bytes(block[h + 1:h + 5], "little"))
    return out


def uint_encoding(block: bytes, at: int) -> str:
    """The Uint encoding byte at `at`: the width, 'd' appended for a delta base."""
    e = block[at]
    return f"{e & 0x7f}{'d' if e & 0x80 else ''}"


def describe(block: bytes, schema: int, tiering: bool = False) -> dict:
    """What the block's header says of it: rows, key_end (the page start of the
    values column: the end of what the decode calls the key region), tail_bytes
    (block length minus the page start of isValueExternal: the two last bitmaps
    and what follows), and per column its encoding: a Uint column's width and
    delta bit ('4', '2d'), the offsets' encoding for RawBytes and PrefixBytes
    (one byte later for PrefixBytes, whose first byte is the bundle shift),
    'zero' or 'bits' for a bitmap."""
    c0 = custom_header(schema)
    pages = column_pages(block, schema, tiering)
    d = {"schema": SCHEMA_NAME[schema], "len": len(block),
         "rows": int.from_bytes(block[c0 + 3:c0 + 7], "little"),
         "key_end": pages["values"][1], "tail_bytes": len(block) - pages["external"][1]}
    for name, (dt, start) in pages.items():
        if dt == DT_BOOL:
            d[name] = "zero" if block[start] == 1 else "bits"
        elif dt == DT_PREFIX:
            d["bundle"] = 1 << block[start]
            d[name] = uint_encoding(block, start + 1)
        else:
            d[name] = uint_encoding(block, start)
        d[name + "_at"] = start
    return d


def context(d: dict) -> str:
    """A failure's context: schema, column encodings and key_end of a block."""
    cols = " ".join(f"{k}={v}" for k, v in d.items()
                    if not k.endswith("_at") and k not in ("schema", "len", "rows", "key_end", "tail_bytes"))
    return f"schema={d['schema']} rows={d['rows']} key_end={d['key_end']} tail_bytes={d['tail_bytes']} {cols}"


# ---- the directed generator ------------------------------------------------------------
WALL0 = 1_700_000_000_000_000_000  # an MVCC wall time of today (ns)
KINDS = (0, 1, 2, 7, 18, 23)


def _alphabet(schema: int, n: int) -> bytes:
    """`n` byte values spread over the whole range, 0x00 and 0xff included; the
    default schema's Split is the first '@', which stays out of its prefixes."""
    vals = sorted({round(i * 255 / (n - 1)) for i in range(n)})
    return bytes(v for v in vals if schema == SCHEMA_CRDB1 or v != 0x40)


def _rand(rng: random.Random, alpha: bytes, n: int) -> bytes:
    return rng.randbytes(n) if len(alpha) == 256 else bytes(rng.choices(alpha, k=n))


def _forced(rng: random.Random, lo: int, hi: int):
    """lo, hi, then random values of [lo, hi]: the first two rows that draw pin
    the column's minimum and maximum, so the range alone decides the encoding."""
    yield lo
    yield hi
    while True:
        yield rng.randint(lo, hi)


def directed_rows(rng: random.Random, schema: int, n: int, *, key_len=(3, 8), alphabet=256, shared=0, dup=0.0,
                  dup_at=(), wall=(WALL0, 3_000_000_000), logical=(0, 0), zero_wall=0.0, untyped=(0.0, (1, 7)),
                  empty=0.0, suffix_len=(1, 3), no_suffix=0.0, seq=(0, 1 << 20), kinds=KINDS, val_len=(0, 8),
                  ext=0.0, obs=0.0):
    """`n` sorted rows (key, trailer, value, value_kind, obsolete), each knob
    forcing one column's encoding:

      key_len, alphabet, shared   key length range, distinct byte values (key
                                  entropy) and a prefix all keys share: the
                                  prefix offsets' width (crdb1: the roach key
                                  before the 0x00 sentinel)
      dup, dup_at                 share / row indices of rows that repeat the
                                  previous row's prefix (duplicate runs)
      wall = (base, span)         crdb1 wall times in [base, base + span]
      logical = (lo, hi)          crdb1 logical values
      zero_wall                   share of MVCC rows with wall 0 (with a logical
                                  value != 0 they stay MVCC rows: cockroachkvs
                                  never writes them, the format holds them)
      untyped = (share, (lo, hi)) crdb1 untyped versions of lo..hi bytes (<= 254)
      empty                       crdb1 share of keys without a version
      suffix_len, no_suffix       default schema: '@' + lo..hi bytes / share of
                                  keys without a suffix
      seq = (base, span), kinds   the trailers: sequence numbers of [base,
                                  base + span] and the set of kinds
      val_len, ext, obs           value length range, share of external values
                                  (block / blob handles), share of obsolete rows
    """
    alpha = _alphabet(schema, alphabet)
    pre = _rand(rng, alpha, shared)
    is_dup = [i > 0 and (i in dup_at or rng.random() < dup) for i in range(n)]
    roots = set()
    while len(roots) < n - sum(is_dup):
        roots.add(pre + _rand(rng, alpha, rng.randint(*key_len)))
    roots = sorted(roots)
    walls, logicals = _forced(rng, wall[0], wall[0] + wall[1]), _forced(rng, *logical)
    seqs = _forced(rng, seq[0], seq[0] + seq[1])
    rows, root = [], -1
    for i in range(n):
        root += not is_dup[i]
        r = roots[root]
        if schema == SCHEMA_CRDB1:
            x = rng.random()
            if x < empty:
                key = r + b"\x00"
            elif x < empty + untyped[0]:
                m = rng.randint(*untyped[1])
                while m in (8, 12, 13):  # (a length byte of 9, 13 or 14 is an MVCC version)
                    m = rng.randint(*untyped[1])
                key = r + b"\x00" + rng.randbytes(m) + bytes([m + 1])
            else:
                w = 0 if rng.random() < zero_wall else next(walls)
                lg = next(logicals)
                if lg == 0:
                    key = r + b"\x00" + struct.pack(">Q", w) + b"\x09"
                elif rng.random() < 0.1:
                    key = r + b"\x00" + struct.pack(">QIB", w, lg, 1) + b"\x0e"  # synthetic bit
                else:
                    key = r + b"\x00" + struct.pack(">QI", w, lg) + b"\x0d"
        elif rng.random() < no_suffix:
            key = r
        else:
            key = r + b"@" + rng.randbytes(rng.randint(*suffix_len))
        kind = kinds[0] if i == 0 else kinds[-1] if i == 1 else rng.choice(kinds)
        vk = VALUE_IN_PLACE
        if rng.random() < ext:
            vk = rng.choice([VALUE_BLOCK_HANDLE, VALUE_BLOB_HANDLE])
        v = rng.randbytes(rng.randint(*val_len))
        rows.append((key, (next(seqs) << 8) | kind, v, vk, rng.random() < obs))
    return rows


def key_prefix(schema: int, key: bytes) -> bytes:
    """The part of a written key that the prefix column holds."""
    if schema == SCHEMA_CRDB1:
        return key[:len(key) - key[-1] - 1]
    i = key.find(b"@")
    return key if i < 0 else key[:i]


def lengthen(schema: int, rows: list, i: int, by: int = 1) -> list:
    """rows with row i's prefix `by` bytes longer (0xff bytes: a last row stays last)."""
    key, *rest = rows[i]
    pl = len(key_prefix(schema, key))
    out = list(rows)
    out[i] = (key[:pl] + b"\xff" * by + key[pl:], *rest)
    return out


# ---- the matrix ---------------------------------------------------------------------------
@dataclass
class Cell:
    name: str
    schema: int
    rows: list        # the writer's input
    bundle: int
    block: bytes
    exp: list         # colutil.build_block's expectation
    desc: dict        # describe(block)
    metas: list = field(default_factory=list)  # expected KVMeta per row (tiering blocks)
    tiering: bool = False

    @property
    def ctx(self) -> str:
        return f"{self.name}: {context(self.desc)}"


THRESHOLDS = (6144, 8192, 12288)   # key_end <= nst: wave size / fixed emit, varlen emit, pipe and single (kStage)
TAIL_STAGE = 512                   # kTail
ROW_COUNTS = (1, 63, 64, 65, 4096, 4097)
BUNDLES = (1, 2, 16, 64)
TRAILER_ENCODINGS = ("0d", "1", "1d", "2d", "4", "4d", "8")
WALL_ENCODINGS = ("0", "0d", "1d", "2d", "4d", "8")
LOGICAL_ENCODINGS = ("0", "1", "2", "4")
TIER_WIDTHS = (0, 1, 2, 4, 8)
REGION_ENCODINGS = {"trailers": ("1d", "4d", "8"), "wall": ("4d", "8")}  # each staged and in global memory

# trailers: sequence-number range and kinds per encoding (>= 8 rows: a delta
# encoding needs UintEncodingRowThreshold rows)
SEQ = {"0d": dict(seq=(5, 0), kinds=(1,)),          # one trailer on every row
       "1": dict(seq=(0, 0)),                        # sequence number 0: a bottom-level compaction's output
       "1d": dict(seq=(7, 0)),                       # one sequence number, several kinds
       "2d": dict(seq=(1 << 30, 200)),
       "4": dict(seq=(0, 1 << 20)),
       "4d": dict(seq=(1 << 40, 1 << 20)),
       "8": dict(seq=(1, (1 << 56) - 2))}            # spread over the whole 56 bits: every trailer byte in use
WALL = {"0d": (WALL0, 0), "1d": (WALL0, 200), "2d": (WALL0, 50_000), "4d": (WALL0, 3_000_000_000),
        "8": (WALL0, 1 << 40)}
LOGICAL = {"0": (0, 0), "1": (0, 200), "2": (0, 50_000), "4": (0, 3_000_000_000)}


def _specs(schema: int):
    """(name, rows, bundle, directed_rows knobs) of the blocks that are not searched for."""
    crdb = schema == SCHEMA_CRDB1
    tiny = dict(key_len=(1, 2), val_len=(0, 0), no_suffix=1.0)  # prefix offsets 1, suffix / untyped 0, values 0
    S = [
        # row counts at the bitmap word boundary, each with other widths
        ("rows1", 1, 16, dict(tiny, wall=WALL["0d"], kinds=(1,), **SEQ["1"])),
        ("rows63", 63, 16, dict(tiny, wall=WALL["1d"], logical=LOGICAL["1"], obs=0.3, **SEQ["0d"])),
        ("rows64", 64, 16, dict(wall=WALL["2d"], logical=LOGICAL["2"], untyped=(0.0, (1, 7)), suffix_len=(4, 9),
                                val_len=(0, 3), ext=0.3, **SEQ["1"])),
        ("rows65", 65, 16, dict(wall=WALL["4d"], logical=LOGICAL["1"], val_len=(2, 9), ext=0.3, obs=0.3, **SEQ["1d"])),
        # the remaining trailer and wall x logical encodings in small blocks (key_end <= 6144)
        ("small_4d", 40, 16, dict(wall=WALL["8"], logical=LOGICAL["4"], val_len=(10, 30), **SEQ["4d"])),
        ("small_8", 40, 16, dict(wall=WALL["4d"], val_len=(10, 30), obs=0.2, **SEQ["8"])),
        ("small_2d", 50, 16, dict(zero_wall=1.0, logical=(1, 200), untyped=(0.4, (1, 5)), empty=0.1,
                                  suffix_len=(1, 3), val_len=(0, 4), **SEQ["2d"])),
        ("small_4", 50, 16, dict(wall=WALL["0d"], val_len=(0, 4), **SEQ["4"])),
        # the same widths past every stage: > 12288 bytes of keys in front of the column
        ("global_1d", 30, 16, dict(key_len=(450, 550), wall=WALL["4d"], logical=LOGICAL["1"], val_len=(40, 80),
                                   **SEQ["1d"])),
        ("global_4d", 30, 16, dict(key_len=(450, 550), wall=WALL["8"], logical=LOGICAL["4"], val_len=(40, 80),
                                   ext=0.2, **SEQ["4d"])),
        ("global_8", 30, 16, dict(key_len=(450, 550), wall=WALL["2d"], val_len=(40, 80), obs=0.2, **SEQ["8"])),
        # 4-byte offsets
        ("prefix_off4", 70, 16, dict(key_len=(1000, 1000), val_len=(0, 4), **SEQ["4"])),
        ("suffix_off4", 300, 16, dict(untyped=(1.0, (240, 254)), suffix_len=(240, 253), val_len=(0, 4),
                                      **SEQ["4"])),
        ("values_off4", 70, 16, dict(val_len=(900, 1100), ext=0.1, **SEQ["4"])),
        # a second bitmap summary word; with both bitmaps set the two last
        # bitmaps pass the 512-byte tail stage
        ("rows4096", 4096, 16, dict(key_len=(2, 3), no_suffix=0.5, empty=0.5, val_len=(0, 0), obs=0.1, **SEQ["1"])),
        ("rows4097", 4097, 16, dict(key_len=(2, 3), no_suffix=0.5, empty=0.5, val_len=(0, 1), ext=0.1,
                                    **SEQ["1d"])),
        ("rows4200", 4200, 16, dict(key_len=(2, 4), dup=0.2, untyped=(0.3, (1, 7)), val_len=(0, 2), ext=0.2, obs=0.2,
                                    **SEQ["4"])),
    ]
    # duplicate runs across a bundle boundary (the rowSuffixOffsets walk-back of
    # row_parts); the crdb1 writer's bundles are always 16
    for b in ((16,) if crdb else BUNDLES):
        at = {k * b + j for k in range(1, 4) for j in (0, 1, 2)}
        S.append((f"bundle{b}", max(3 * b + 8, 40), b, dict(dup=0.15, dup_at=at, alphabet=4, shared=3, val_len=(0, 6),
                                                            **SEQ["4"])))
    return S


def _threshold_cells(schema: int):
    """Per threshold T a block with key_end == T and one with key_end == T + 8:
    a prefix of a fixed row list that ends just under T, its last key then
    lengthened a byte at a time (key_end follows the prefixChanged bitmap's
    words, so it moves in steps of 8)."""
    rng = random.Random(900 + schema)
    pool = directed_rows(rng, schema, 900, key_len=(8, 24), wall=WALL["4d"], logical=LOGICAL["1"], val_len=(0, 12),
                         ext=0.1, obs=0.1, **SEQ["4"])
    key_end = lambda rows: describe(build_block(schema, rows)[0], schema)["key_end"]  # noqa: E731
    for T in THRESHOLDS:
        lo, hi = 1, len(pool)  # the most rows whose key_end stays under T
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if key_end(pool[:mid]) < T else (lo, mid - 1)
        rows = pool[:lo]
        for want in (T, T + 8):
            while key_end(rows) < want:
                rows = lengthen(schema, rows, len(rows) - 1)
            assert key_end(rows) == want, (schema, want, key_end(rows))
            yield f"key_end{want}", rows


def _make(name: str, schema: int, rows: list, bundle: int = 16) -> Cell:
    blk, exp = build_block(schema, rows, bundle)
    return Cell(f"{SCHEMA_NAME[schema]}/{name}", schema, rows, bundle, blk, exp, describe(blk, schema))


@functools.lru_cache(maxsize=None)
def matrix() -> tuple:
    """Every cell of the matrix, both schemas (built once)."""
    cells = []
    for schema in (SCHEMA_DEFAULT, SCHEMA_CRDB1):
        for i, (name, n, bundle, knobs) in enumerate(_specs(schema)):
            rows = directed_rows(random.Random(1000 * schema + i), schema, n, **knobs)
            cells.append(_make(name, schema, rows, bundle))
        for name, rows in _threshold_cells(schema):
            cells.append(_make(name, schema, rows))
    return tuple(cells)


def _tier_values(rng: random.Random, n: int, width: int, nonzero: bool) -> list:
    """n values whose Uint column takes `width` bytes (the writer's default is 0,
    so there is no delta): the first row holds the widest value."""
    if width == 0:
        return [0] * n
    top = (1 << 8 * width) - 1
    return [top] + [rng.randint(1 if nonzero else 0, top) for _ in range(n - 1)]


@functools.lru_cache(maxsize=None)
def tiering_matrix() -> tuple:
    """Pebblev8 blocks (tiering columns) over the threshold blocks and the
    4200-row block, so that the tiering columns lie past every stage; span and
    attribute widths 0, 1, 2, 4 and 8 (an attribute of 0 is an unset KVMeta, so
    the attribute width 0 comes with span width 0)."""
    widths = [(0, 1), (1, 2), (2, 4), (4, 8), (8, 1), (0, 0), (1, 8), (2, 2)]
    cells = []
    for schema in (SCHEMA_DEFAULT, SCHEMA_CRDB1):
        base = [c for c in matrix() if c.schema == schema and ("key_end" in c.name or "rows4200" in c.name)]
        for i, c in enumerate(base):
            rng = random.Random(7000 + 10 * schema + i)
            sw, aw = widths[(i + schema) % len(widths)]
            n = len(c.rows)
            attrs = _tier_values(rng, n, aw, True)
            attrs = [a if j == 0 or rng.random() < 0.8 else 0 for j, a in enumerate(attrs)]  # a fifth unset
            metas = list(zip(_tier_values(rng, n, sw, False), attrs))
            blk, exp, em = build_block_meta(schema, c.rows, metas, c.bundle)
            cells.append(Cell(f"{c.name}/span{sw}attr{aw}", schema, c.rows, c.bundle, blk, exp,
                              describe(blk, schema, True), em, True))
    return tuple(cells)


# ---- negative cases ----------------------------------------------------------------------------
def _with_byte(block: bytes, at: int, v: int) -> bytes:
    b = bytearray(block)
    b[at] = v
    return bytes(b)


def _with_offsets_base(block: bytes, schema: int, col: str, base: int) -> bytes:
    """The block with a delta base in front of `col`'s offsets: the encoding
    byte's delta bit, eight base bytes, and every later page eight bytes on
    (all alignments hold)."""
    pages = column_pages(block, schema)
    start = pages[col][1] + (pages[col][0] == DT_PREFIX)
    b = bytearray(block[:start + 1] + base.to_bytes(8, "little") + block[start + 1:])
    b[start] |= 0x80
    c0 = custom_header(schema)
    for i, name in enumerate(column_names(schema)):
        if pages[name][1] > start:
            h = c0 + 7 + 5 * i
            b[h + 1:h + 5] = (pages[name][1] + 8).to_bytes(4, "little")
    return bytes(b)


@functools.lru_cache(maxsize=None)
def negatives() -> tuple:
    """(name, schema, block, the valid cell it was made from): a Uint column's
    encoding byte set to width 8 with a delta base and to the widths 3 and 16;
    an offsets column with a delta base (zero and non-zero); the row count
    raised by one.  Each one's status is the oracle's to say (it takes a zero
    base on offsets: such a block decodes to what its source does)."""
    out = []
    for schema in (SCHEMA_DEFAULT, SCHEMA_CRDB1):
        by_name = {c.name.split("/", 1)[1]: c for c in matrix() if c.schema == schema}
        for src in ("small_8", "rows65", "global_4d"):
            c = by_name[src]
            for col in ("trailers",) + (("wall", "logical") if schema == SCHEMA_CRDB1 else ()):
                for enc in (8 | 0x80, 3, 16):
                    out.append((f"{c.name}/{col}=enc{enc:#x}", schema, _with_byte(c.block, c.desc[col + "_at"], enc), c))
            for col in ("values", "prefix", "untyped" if schema == SCHEMA_CRDB1 else "suffix"):
                for base in (0, 1):
                    out.append((f"{c.name}/{col}+base{base}", schema, _with_offsets_base(c.block, schema, col, base), c))
            at = custom_header(schema) + 3
            rows = (c.desc["rows"] + 1).to_bytes(4, "little")
            out.append((f"{c.name}/rows+1", schema, c.block[:at] + rows + c.block[at + 4:], c))
    return tuple(out)


# ---- what the matrix covers ---------------------------------------------------------------------
OFFSET_COLUMN = {SCHEMA_DEFAULT: "suffix", SCHEMA_CRDB1: "untyped"}


def has_crossing_run(c: Cell) -> bool:
    """A run of equal prefixes that reaches over a bundle boundary and on: the
    bundle's first row holds its suffix again, the row after it does not."""
    p = [key_prefix(c.schema, r[0]) for r in c.rows]
    return any(p[i - 1] == p[i] == p[i + 1] for i in range(c.bundle, len(p) - 1, c.bundle))


def coverage(cells, tier_cells) -> dict:
    """The cells the blocks reach, from describe() and the writer's input alone."""
    enc, pairs, regions, thresholds, row_counts, big, bundles = set(), set(), set(), set(), set(), set(), set()
    for c in cells:
        d, s = c.desc, SCHEMA_NAME[c.schema]
        cols = ["trailers", "prefix", OFFSET_COLUMN[c.schema], "values", "external", "obsolete"]
        if c.schema == SCHEMA_CRDB1:
            cols += ["wall", "logical"]
            pairs.add((d["wall"], d["logical"]))
        enc |= {(s, col, d[col]) for col in cols}
        for col, encs in REGION_ENCODINGS.items():
            if d.get(col) not in encs:
                continue
            if d["key_end"] <= THRESHOLDS[0]:
                regions.add((s, col, d[col], "staged"))
            # read from global memory on every route: the whole column past the
            # largest head stage and in front of the staged tail
            end = d[col + "_at"] + 9 + d["rows"] * int(d[col].rstrip("d"))
            if d["key_end"] > THRESHOLDS[-1] <= d[col + "_at"] and end <= (d["len"] - TAIL_STAGE) & ~15:
                regions.add((s, col, d[col], "global"))
        if d["key_end"] in [t + k for t in THRESHOLDS for k in (0, 8)]:
            thresholds.add((s, d["key_end"]))
        if d["rows"] in ROW_COUNTS:
            row_counts.add((s, d["rows"]))
        if d["rows"] >= 4200 and d["external"] == d["obsolete"] == "bits" and d["tail_bytes"] > TAIL_STAGE:
            big.add(s)
        if c.schema == SCHEMA_DEFAULT and has_crossing_run(c):
            bundles.add(d["bundle"])
    tier = {(col, c.desc[col]) for c in tier_cells for col in ("span", "attr")}
    return dict(encodings=enc, wall_logical=pairs, regions=regions, thresholds=thresholds, row_counts=row_counts,
                two_summary_words=big, bundles=bundles, tiering=tier)


def required_coverage() -> dict:
    """Section by section, the cells the matrix must hold -- no more, no fewer."""
    enc, regions = set(), set()
    for schema, s in SCHEMA_NAME.items():
        enc |= {(s, "trailers", e) for e in TRAILER_ENCODINGS}
        enc |= {(s, "prefix", e) for e in ("1", "2", "4")}
        enc |= {(s, col, e) for col in (OFFSET_COLUMN[schema], "values") for e in ("0", "1", "2", "4")}
        enc |= {(s, col, e) for col in ("external", "obsolete") for e in ("zero", "bits")}
        regions |= {(s, "trailers", e, r) for e in REGION_ENCODINGS["trailers"] for r in ("staged", "global")}
    enc |= {("crdb1", "wall", e) for e in WALL_ENCODINGS} | {("crdb1", "logical", e) for e in LOGICAL_ENCODINGS}
    regions |= {("crdb1", "wall", e, r) for e in REGION_ENCODINGS["wall"] for r in ("staged", "global")}
    names = SCHEMA_NAME.values()
    return dict(encodings=enc, regions=regions,
                thresholds={(s, t + k) for s in names for t in THRESHOLDS for k in (0, 8)},
                row_counts={(s, n) for s in names for n in ROW_COUNTS}, two_summary_words=set(names),
                bundles=set(BUNDLES), tiering={(col, str(w)) for col in ("span", "attr") for w in TIER_WIDTHS})
