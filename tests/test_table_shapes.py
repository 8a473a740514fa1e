"""tests/tableshapeutil.py held to the oracle and to the reference's own bytes
(CPU): what makes the expectations of tests/test_table_shapes_gpu.py
trustworthy.  Every generated block decodes, through the oracle, back to the
rows it was built from; forced encodings are really in the bytes; the encoder
reproduces the reference's printed index blocks byte for byte; the synthetic
table scans to its construction list; and the census of the case lists is
exactly the required one."""
import json
import os

import oracle
import tableshapeutil as U
from tableutil import table_bytes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEMPLATE = "cr_schema_000014.sst"


def test_index_col_blocks_decode_to_their_rows():
    for name, blk, rows in U.index_col_shape_cases():
        st, got = oracle.index_block_col(blk)
        assert st == 0 and got == [tuple(r) for r in rows], name
    blocks, rows = U.index_col_pool()
    assert len(blocks) == U.GRID + 1
    for i in list(range(0, len(blocks), 97)) + [len(blocks) - 1]:
        assert oracle.index_block_col(blocks[i]) == (0, [tuple(r) for r in rows[i]]), i


def test_forced_index_encodings_are_in_the_bytes():
    seen = set()
    for name, blk, _rows in U.index_col_shape_cases():
        if name.startswith("off") and "_len" in name:
            fo, fl = name[3:].split("_len")
            assert (U.uint_encoding(blk, 1), U.uint_encoding(blk, 2)) == (fo, fl), name
            seen |= {("o", fo), ("l", fl)}
    assert seen == {(c, f) for c in "ol" for f in U.UINT_FORMS}
    by = {name: blk for name, blk, _ in U.index_col_shape_cases()}
    # what the writer picks on its own: a file past 64 KiB / 4 GiB, equal lengths, the props' offsets
    assert (U.uint_encoding(by["file64k"], 1), U.uint_encoding(by["file64k"], 2)) == ("4", "0d")
    assert U.uint_encoding(by["file4g"], 1) == "8"
    assert [U.uint_encoding(by[n], 3) for n in ("props_empty", "props300", "props70000")] == ["0", "2", "4"]
    kv = {name: blk for name, blk, _ in U.kv_shape_cases()}
    assert [U.uint_encoding(kv[n], 1) for n in ("rows63", "off2", "off4", "values_empty")] == ["1", "2", "4", "0"]
    assert (U.uint_encoding(kv["forced_off4"], 0), U.uint_encoding(kv["forced_off4"], 1)) == ("4", "2")
    assert U.uint_encoding(kv["keys_empty"], 0) == "0"


def test_malformed_index_blocks_are_rejected_by_the_oracle():
    good, bad = U.index_col_malformed()
    assert oracle.index_block_col(good)[0] == 0
    for name, blk in bad:
        assert oracle.index_block_col(blk)[0] == U.CORRUPT_HEADER, name


def test_encoder_reproduces_the_reference_index_blocks():
    """Byte for byte, from the rows of each index block the reference prints
    (colblk/testdata/index_block).  A block the reference finished with fewer
    rows than it added (`build rows=N`) keeps what Finish(rows) leaves of the
    unwritten rows: it is compared too and must come out the same."""
    with open(os.path.join(GOLDEN, "sstable.json")) as f:
        fix = json.load(f)
    assert len(fix["index_blocks"]) == 6
    for c in fix["index_blocks"]:
        rows = [(r[0].encode(), r[1], r[2], r[3].encode()) for r in c["rows"]]
        assert U.col_index_block(rows).hex() == c["block_hex"], c["cmd"]


def test_row_index_blocks_decode_to_their_entries():
    for name, blk, ents in U.index_row_shape_cases():
        assert oracle.index_block_row(blk) == (0, [tuple(e) for e in ents]), name
    for name, blk in U.index_row_corrupt_cases():
        assert oracle.index_block_row(blk) == (U.CORRUPT_INDEX, []), name
    blocks, ents = U.index_row_pool()
    for i in list(range(0, len(blocks), 331)) + [len(blocks) - 1]:
        assert oracle.index_block_row(blocks[i]) == (0, [tuple(ents[i])]), i
    assert oracle.index_block_row(U.corrupt_row_block())[0] == 1  # PBL_CORRUPT_NO_RESTARTS
    # 2^64 - 1 in both fields, ten bytes each
    assert any(o == U.U64 for _n, _b, es in U.index_row_shape_cases() for o, _l, _p in es)
    assert any(ln == U.U64 for _n, _b, es in U.index_row_shape_cases() for _o, ln, _p in es)


def test_kv_blocks_decode_to_their_rows():
    for name, blk, rows in U.kv_shape_cases():
        assert oracle.kv_block_col(blk) == (0, [tuple(r) for r in rows]), name
    blocks, rows = U.kv_pool()
    for i in list(range(0, len(blocks), 331)) + [len(blocks) - 1]:
        assert oracle.kv_block_col(blocks[i]) == (0, [tuple(r) for r in rows[i]]), i
    for name, blk in U.kv_corrupt_cases():
        want = U.CORRUPT_HEADER if name.startswith("last_past_block") else U.CORRUPT_BOUNDS
        assert oracle.kv_block_col(blk) == (want, []), name


def test_valblk_index_restatement():
    for name, data, w in U.valblk_cases():
        hs, err = U.decode_valblk_index(data, w)
        if name.startswith(("wrong_num", "ragged")):
            assert hs is None and err, name
        else:
            assert hs == U.valblk_handles(len(data) // sum(w), w), name


def test_value_handles_name_their_values():
    """Canonical handles under the reference's five-byte rule (valblk.go:206-279)
    and Go's Uvarint agree: the construction list is what both read."""
    vbs = U.value_blocks()
    rows, cols, kvs = U.resolve_shape_cases()
    for blk, ks in zip(rows, kvs):
        st, got, _ = oracle.rowblk_decode_block(blk, 0x1)
        assert st == 0 and len(got) == len(ks)
        for (_k, _t, v, fl, _e), (_i, inplace, h, exp) in zip(got, ks):
            if h is None:
                assert not fl & 0x10 and v == inplace == exp
                continue
            assert fl & 0x10 and v == U.value_handle(*h)
            vlen, a = oracle.go_uvarint(v, 1)
            bn, c = oracle.go_uvarint(v, 1 + a)
            off, d = oracle.go_uvarint(v, 1 + a + c)
            assert max(a, c, d) <= 5 and 1 + a + c + d == len(v)  # (within the reference's five bytes)
            assert (vlen, bn, off) == h == U.ref_decode_handle(v[1:])
            assert vbs[bn][off:off + vlen] == exp and len(exp) == vlen
    for blk, ks in zip(cols, kvs):
        st, got = oracle.colblk_decode_block(blk, 2)
        assert st == 0 and [bool(r[3] & 0x10) for r in got] == [k[2] is not None for k in ks]
    # every handle of the large batches and of the table, under both rules
    hs = [k[2] for ks in U.resolve_pool("row")[1] for k in ks if k[2] is not None]
    _data, info = U.synthetic_table(table_bytes(TEMPLATE))
    hs += [U.ALIAS_VALUE] + [U.ref_decode_handle(s) for s, is_handle in info["stored"] if is_handle]
    for h in hs:
        v = U.value_handle(*h)
        vlen, a = oracle.go_uvarint(v, 1)
        bn, c = oracle.go_uvarint(v, 1 + a)
        off, d = oracle.go_uvarint(v, 1 + a + c)
        assert (vlen, bn, off) == h == U.ref_decode_handle(v[1:]) and min(a, c, d) > 0, h
        assert off + vlen <= len(vbs[bn])
    # the non-canonical forms are where the two rules part: the
    # reference reads a field padded to six bytes as five bytes and goes on in
    # the middle of it; Go's Uvarint reads the value
    cases = {n: raw for n, raw, _e in U.resolve_corrupt_cases()}
    assert U.ref_decode_handle(cases["six_byte_len_padded"]) != (5, 7, 0)
    assert [oracle.go_uvarint(cases["six_byte_len_padded"], 0), oracle.go_uvarint(cases["eleven_byte_len"], 0)[1] < 0,
            oracle.go_uvarint(cases["tenth_byte_2"], 0)[1] < 0] == [(5, 6), True, True]


def test_synthetic_table_scans_to_its_construction_list():
    data, info = U.synthetic_table(table_bytes(TEMPLATE))
    assert len(info["data_handles"]) > U.GRID and len(info["lower"]) > U.SCAN and info["top_rows"] > U.TPB
    assert info["n_value_blocks"] > 129
    assert len(data) < 1 << 24  # the value index's 3-byte offsets
    props, kvs = oracle.table_scan(data)
    assert props[b"pebble.colblk.schema"] == b"crdb1"
    assert [(k, t, v) for k, t, v, _fl in kvs] == info["kvs"]
    assert [bool(fl & 0x10) for _k, _t, _v, fl in kvs] == [h for _s, h in info["stored"]]


def test_census_is_the_required_one():
    got, want = U.census(), U.required_census()
    assert set(got) == set(want)
    for entry in want:
        assert got[entry] == want[entry], (entry, got[entry] ^ want[entry])
