"""The directed colblk matrix (tests/colencutil.py) on the CPU: describe() reads
the encodings the reference's own dumps name, the matrix covers exactly the
cells it is meant to (every Uint width and delta bit per column, both sides of
each stage threshold, the bitmap word boundaries, duplicate runs across bundle
boundaries, the tiering widths), every block decodes in the oracle to what the
writer was given, and the negative blocks' statuses are the oracle's.
tests/test_colblk_encodings_gpu.py decodes the same blocks on every device route."""
import json
import os
import re

import oracle
from colencutil import (DT_PREFIX, THRESHOLDS, column_pages, coverage, describe, matrix, negatives,
                        required_coverage, tiering_matrix)
from pebble_amd import _native as N
from pebble_amd.colblk import SCHEMA_CRDB1, SCHEMA_DEFAULT

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "colblk_golden.json")


def dump_encoding(dump: str) -> str:
    """The encoding a codec fixture's dump names, in describe()'s spelling."""
    if "zero bitmap encoding" in dump:
        return "zero"
    if "default bitmap encoding" in dump:
        return "bits"
    m = re.search(r"# encoding: (zero|\d+b)(,delta)?", dump)
    return ("0" if m.group(1) == "zero" else m.group(1)[:-1]) + ("d" if m.group(2) else "")


def test_describe_agrees_with_the_codec_dumps():
    from test_oracle_codecs import embedded_blocks
    col = {"uints": "trailers", "raw_bytes": "values", "bitmap": "obsolete", "prefix_bytes": "prefix"}
    seen = set()
    for codec, e, blk in embedded_blocks():
        d = describe(blk, SCHEMA_DEFAULT)
        assert d["rows"] == e["rows"], e["source"]
        assert d[col[codec]] == dump_encoding(e["dump"]), (e["source"], d)
        if codec == "prefix_bytes":
            assert d["bundle"] == int(re.search(r"# bundle size: (\d+)", e["dump"]).group(1)), e["source"]
        seen.add((codec, d[col[codec]]))
    assert {("uints", w) for w in ("0", "1", "2", "4", "8", "4d")} <= seen
    assert {("bitmap", "zero"), ("bitmap", "bits"), ("prefix_bytes", "2")} <= seen


def uint_column(block: bytes, at: int, rows: int) -> list:
    """A Uint column's values in plain Python, from the encoding byte at `at`."""
    w, delta = block[at] & 0x7f, block[at] >> 7
    base = int.from_bytes(block[at + 1:at + 9], "little") if delta else 0
    o = at + 1 + 8 * delta
    o = (o + w - 1) // w * w if w else o
    return [base + int.from_bytes(block[o + i * w:o + (i + 1) * w], "little") for i in range(rows)]


def bitmap_column(block: bytes, at: int, rows: int) -> list:
    if block[at] == 1:
        return [False] * rows
    o = (at + 8) & ~7
    return [bool(block[o + (r >> 3)] >> (r & 7) & 1) for r in range(rows)]


def test_describe_on_the_golden_data_blocks():
    """The data-block fixtures record rows, not dumps: the columns that
    describe() locates, read with the encodings it reports, hold the recorded
    trailers and bitmaps (the tiering blocks: the recorded KVMeta too)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    seen = set()
    for c in g["data_blocks"] + g["tiering"]["blocks"]:
        schema = SCHEMA_CRDB1 if c["schema"] == "crdb1" else SCHEMA_DEFAULT
        blk, rows, tier = bytes.fromhex(c["block"]), c["rows"], "span" in c["rows"][0]
        d = describe(blk, schema, tier)
        assert d["rows"] == len(rows) and d["bundle"] == c["bundle_size"], c["name"]
        assert uint_column(blk, d["trailers_at"], len(rows)) == [r["trailer"] for r in rows], c["name"]
        for col, key in (("external", "external"), ("obsolete", "obsolete"), ("prefix_changed", "prefix_changed")):
            assert bitmap_column(blk, d[col + "_at"], len(rows)) == [bool(r[key]) for r in rows], (c["name"], col)
        if tier:
            for col in ("span", "attr"):
                assert uint_column(blk, d[col + "_at"], len(rows)) == [r[col] for r in rows], (c["name"], col)
        assert d["key_end"] == column_pages(blk, schema, tier)["values"][1] < len(blk) - d["tail_bytes"] + 1
        seen.add(d["trailers"])
    assert {"0d", "1", "2"} <= seen  # (what the issue's count found in the golden blocks)


def test_matrix_covers_every_cell():
    """Asserted, not hoped for: an edit of the generator that loses a cell (or
    reaches an encoding the list does not name) fails here."""
    cov, req = coverage(matrix(), tiering_matrix()), required_coverage()
    for k, want in req.items():
        assert cov[k] == want, (k, "missing", sorted(want - cov[k]), "not listed", sorted(cov[k] - want))
    assert {("4d", "1"), ("8", "4")} <= cov["wall_logical"]
    # the tiering columns lie past the values: past the 6144-byte
    # stage in every block, past the 8192- and 12288-byte ones in most
    at = [c.desc["span_at"] for c in tiering_matrix()]
    assert min(at) > THRESHOLDS[0] and sum(a > THRESHOLDS[2] for a in at) >= 4
    # keys use the whole byte range, and wall 0 comes with a logical value
    crdb = [c for c in matrix() if c.schema == SCHEMA_CRDB1]
    assert {0x00, 0xff} <= {b for c in crdb for r in c.rows[:50] for b in r[0][:len(r[0]) - r[0][-1] - 1]}
    assert any(r[0][-1] == 13 and r[0][-13:-5] == bytes(8) and r[0][-5:-1] != bytes(4) for c in crdb for r in c.rows)
    assert max(len(c.block) for c in matrix()) < 160 << 10


def expected(c):
    return [e[:4] for e in c.exp]


def test_matrix_blocks_decode_in_the_oracle():
    for c in matrix():
        st, kvs = oracle.colblk_decode_block(c.block, c.schema)
        assert st == N.PBL_OK, c.ctx
        assert [kv[:4] for kv in kvs] == expected(c), c.ctx
    for c in tiering_matrix():
        st, kvs = oracle.colblk_decode_block(c.block, c.schema, oracle.FLAG_TIERING, meta=True)
        assert st == N.PBL_OK, c.ctx
        assert [kv[:4] for kv in kvs] == expected(c), c.ctx
        assert [kv[5:] for kv in kvs] == c.metas, c.ctx


def test_negative_blocks_in_the_oracle():
    """A Uint width of 8 with a delta base, and the widths 3 and 16, are not
    encodings (UintEncoding.IsValid); offsets never carry a non-zero base; one
    row more than the columns hold fails the metadata init or the bounds
    checks.  A zero base on offsets is read as no base: the block decodes to
    what its source does."""
    for name, schema, blk, src in negatives():
        st, kvs = oracle.colblk_decode_block(blk, schema)
        if "+base" in name:
            col = name.rsplit("/", 1)[1].split("+")[0]
            dt, start = column_pages(blk, schema)[col]
            assert blk[start + (dt == DT_PREFIX)] & 0x80, name  # (the delta bit is where describe() reads it)
            assert describe(blk, schema)[col] == src.desc[col] + "d", name
        if name.endswith("+base0"):
            assert st == N.PBL_OK and [kv[:4] for kv in kvs] == expected(src), name
        elif "=enc" in name or name.endswith("+base1"):
            assert st == N.PBL_CORRUPT_COLBLK_HEADER, name
        else:
            assert st in (N.PBL_CORRUPT_COLBLK_HEADER, N.PBL_CORRUPT_BOUNDS), name
