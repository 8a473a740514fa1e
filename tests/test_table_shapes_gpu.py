"""The table-layer kernels (pebble_amd/csrc/sstable.hip) and the batch entry
points of physical.hip past one pass of every loop and scan: more than 256
rows in a block, more than 64 entries under one wave, more than 1024, 4096 and
16384 blocks in a batch, every Uint encoding of an index column, every varint
length of a handle field (tests/tableshapeutil.py builds the inputs;
tests/test_table_shapes.py holds them to the oracle and to the census).

Every comparison is exact.  The expected side is the oracle per block or the
list the input was built from, never a second run of the device.  Malformed
inputs stay inside padded allocations.

Not covered: a block whose resolved values pass 4 GiB (PBL_UNSUPPORTED from
pbl_resolve_values) would need gigabytes of value blocks.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import tableshapeutil as U
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, decode
from pebble_amd.physical import PhysBatch, decompress, verify_checksums
from pebble_amd.rowblk import kvs_of_block
from pebble_amd.seek import seek_host
from pebble_amd.sstable import (IndexHandles, KvSlices, Table, index_handles_col, index_handles_row, kv_blocks,
                                resolve_values)
from seekutil import assert_seek, device_result
from tableutil import table_bytes

pytestmark = pytest.mark.gpu
U64 = np.uint64


def batch_of(blocks, align=8, fmt=N.PBL_FMT_ROW, flags=0):
    buf, off, lens = U.pack(list(blocks), align)
    return buf, BlockBatch.from_host(buf, off, lens, "cuda", fmt, flags)


def u64(xs):
    return np.array(list(xs), dtype=U64)


# ---- pbl_index_handles_col ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_col_pool_expected():
    return tuple(oracle.index_block_col(b) for b in U.index_col_pool()[0])


def check_index_col(blocks, expected, align, ctx):
    """index_handles_col over `blocks` against `expected` = [(status, rows)]."""
    buf, bb = batch_of(blocks, align)
    h = index_handles_col(bb)
    counts = [len(rows) if st == 0 else 0 for st, rows in expected]
    base = np.concatenate([[0], np.cumsum(counts)]).astype(U64)
    n = int(base[-1])
    assert np.array_equal(h.status(), np.array([st for st, _ in expected], np.uint32)), ctx
    assert np.array_equal(h.blk_base.cpu().numpy().view(U64), base), ctx
    assert h.total(len(blocks)) == n, ctx
    rows = [r for st, rs in expected if st == 0 for r in rs]
    assert np.array_equal(h.handle_off[:n].cpu().numpy().view(U64), u64(r[1] for r in rows)), ctx
    assert np.array_equal(h.handle_len[:n].cpu().numpy().view(U64), u64(r[2] for r in rows)), ctx
    po, pl = h.props_off[:n].cpu().numpy(), h.props_len[:n].cpu().numpy()
    raw = buf.tobytes()
    assert [raw[o:o + m] for o, m in zip(po.tolist(), pl.tolist())] == [r[3] for r in rows], ctx


def test_index_col_rows_and_encodings():
    """0 .. 1000 rows in a block, offsets and lengths in every Uint form
    (constant, 1 / 2 / 4 / 8 bytes, delta bases above 2^32), props offsets of 0,
    1, 2 and 4 bytes, at both alignments."""
    cases = U.index_col_shape_cases()
    blocks = [c[1] for c in cases]
    expected = [(0, [tuple(r) for r in c[2]]) for c in cases]
    assert expected == [oracle.index_block_col(b) for b in blocks]
    for align in (8, 1):
        check_index_col(blocks, expected, align, f"align {align}")
    for c, e in zip(cases, expected):
        check_index_col([c[1]], [e], 8, c[0])


@pytest.mark.parametrize("n", U.INDEX_COL_BATCHES)
def test_index_col_batches(n):
    """Batches up to a second chunk of the scan and a second pass of the grid;
    packed without padding, so the blocks start at every residue mod 8."""
    blocks, expected = U.index_col_pool()[0][:n], index_col_pool_expected()[:n]
    check_index_col(blocks, expected, 1, f"{n} blocks")


def test_index_col_malformed():
    good, bad = U.index_col_malformed()
    blocks = [good] + [b for _n, b in bad] + [good]
    expected = [oracle.index_block_col(b) for b in blocks]
    assert expected[0][0] == 0 and all(st == N.PBL_CORRUPT_COLBLK_HEADER for st, _ in expected[1:-1])
    for align in (8, 1):
        check_index_col(blocks, expected, align, f"align {align}")


def index_col_raw(bb, cap):
    out = IndexHandles.allocate(bb.n_blocks, cap, "cuda")
    for t in (out.handle_off, out.handle_len):
        t.fill_(-1)
    c = out.c_struct()
    c.cap = cap
    b = bb.c_struct()
    assert N.lib().pbl_index_handles_col(ctypes.byref(b), ctypes.byref(c), None) == 0
    torch.cuda.synchronize()
    return out


def test_index_col_capacity():
    """Capacity exact, one short and zero: exactly the blocks with base + rows >
    cap are PBL_OVERFLOW, the others are written in full, blk_base[n] is the
    true total, and index_handles_col()'s re-run returns everything."""
    cases = U.index_col_shape_cases()
    blocks = [c[1] for c in cases]
    counts = [len(c[2]) for c in cases]
    base = np.concatenate([[0], np.cumsum(counts)])
    total = int(base[-1])
    offs = u64(r[1] for c in cases for r in c[2])
    _buf, bb = batch_of(blocks)
    for cap in (total, total - 1, 0):
        out = index_col_raw(bb, cap)
        want = [N.PBL_OVERFLOW if base[i] + counts[i] > cap else 0 for i in range(len(blocks))]
        assert list(out.status()) == want, cap
        assert np.array_equal(out.blk_base.cpu().numpy(), base), cap
        ho = out.handle_off.cpu().numpy().view(U64)
        for i, st in enumerate(want):
            if st == 0:
                assert np.array_equal(ho[base[i]:base[i + 1]], offs[base[i]:base[i + 1]]), (cap, i)
        first_over = min([base[i] for i, st in enumerate(want) if st] + [max(cap, 1)])
        assert (ho[first_over:max(cap, 1)] == U64(U.U64)).all(), cap  # nothing written for a block that does not fit
    assert want[0] == 0 and want[1] == N.PBL_OVERFLOW  # cap 0: the block without rows fits
    h = index_handles_col(bb, cap=5)
    assert h.total(len(blocks)) == total and not h.status().any()
    assert np.array_equal(h.handle_off[:total].cpu().numpy().view(U64), offs)


# ---- pbl_index_handles_row ---------------------------------------------------------------------
def check_index_row(blocks, expected, ctx):
    """index_handles_row over decoded `blocks` against `expected` =
    [(status, [(off, len, props)])] (oracle.index_block_row)."""
    _buf, bb = batch_of(blocks)
    d = decode(bb)
    src = d.to_host()
    h = index_handles_row(d, len(blocks))
    assert np.array_equal(h.status(), np.array([st for st, _ in expected], np.uint32)), ctx
    base = h.blk_base.cpu().numpy().view(U64)
    assert np.array_equal(base, src["blk_kv_base"]), ctx
    ho, hl = h.handle_off.cpu().numpy().view(U64), h.handle_len.cpu().numpy().view(U64)
    po, pl = h.props_off.cpu().numpy(), h.props_len.cpu().numpy()
    vals = src["val_bytes"].tobytes()
    for b, (st, ents) in enumerate(expected):
        k0, k1 = int(base[b]), int(base[b + 1])
        if st in (0, N.PBL_CORRUPT_INDEX):
            assert k1 - k0 == (len(ents) if st == 0 else int(src["blk_kv_base"][b + 1] - src["blk_kv_base"][b])), (ctx, b)
        else:
            assert k1 == k0, (ctx, b)  # a block the row decode rejects owns no entries
        if st:
            continue
        assert np.array_equal(ho[k0:k1], u64(e[0] for e in ents)), (ctx, b)
        assert np.array_equal(hl[k0:k1], u64(e[1] for e in ents)), (ctx, b)
        assert [vals[o:o + m] for o, m in zip(po[k0:k1].tolist(), pl[k0:k1].tolist())] == [e[2] for e in ents], (ctx, b)


def test_index_row_entries_and_varints():
    """1 .. 300 entries under one wave; offset and length varints of 1 .. 10
    bytes, 2^64 - 1 included; a tenth byte above 1 and an unterminated varint in
    entry 0, in entry 70 and in the last entry: PBL_CORRUPT_INDEX for that block
    alone; a block the row decode rejects keeps its status."""
    blocks = [c[1] for c in U.index_row_shape_cases()]
    corrupt = [b for _n, b in U.index_row_corrupt_cases()]
    mixed = []
    for i, b in enumerate(corrupt):
        mixed += [b, blocks[i % len(blocks)]]
    mixed.insert(3, U.corrupt_row_block())
    expected = [oracle.index_block_row(b) for b in mixed]
    sts = [st for st, _ in expected]
    assert sts.count(N.PBL_CORRUPT_INDEX) == len(corrupt) and sts.count(N.PBL_CORRUPT_NO_RESTARTS) == 1
    check_index_row(blocks, [oracle.index_block_row(b) for b in blocks], "shapes")
    check_index_row(mixed, expected, "corrupt among good")


def test_index_row_batch_past_the_grid():
    blocks, _ents = U.index_row_pool()
    assert len(blocks) > U.WAVE_GRID
    check_index_row(blocks, [oracle.index_block_row(b) for b in blocks], "16385 blocks")


# ---- pbl_kv_blocks --------------------------------------------------------------------------------
def check_kv(blocks, expected, align, ctx):
    buf, bb = batch_of(blocks, align)
    kv = kv_blocks(bb)
    counts = [len(rows) for _st, rows in expected]
    base = np.concatenate([[0], np.cumsum(counts)]).astype(U64)
    n = int(base[-1])
    assert np.array_equal(kv.status(), np.array([st for st, _ in expected], np.uint32)), ctx
    assert np.array_equal(kv.blk_base.cpu().numpy().view(U64), base), ctx
    raw = buf.tobytes()
    ko, kl = kv.key_off[:n].cpu().tolist(), kv.key_len[:n].cpu().tolist()
    vo, vl = kv.val_off[:n].cpu().tolist(), kv.val_len[:n].cpu().tolist()
    got = [(raw[a:a + m], raw[c:c + q]) for a, m, c, q in zip(ko, kl, vo, vl)]
    assert got == [r for _st, rows in expected for r in rows], ctx


def test_kv_rows_and_offsets():
    """0 .. 1000 rows (a second pass of the wave's and of the workgroup's row
    loop), empty keys and values, offsets of 0, 1, 2 and 4 bytes.  A row whose
    offsets decrease is PBL_CORRUPT_BOUNDS for its block, wherever it lies; a
    last offset past the block is the header's PBL_CORRUPT_COLBLK_HEADER."""
    blocks = [c[1] for c in U.kv_shape_cases()]
    corrupt = [b for _n, b in U.kv_corrupt_cases()]
    mixed = []
    for i, b in enumerate(corrupt):
        mixed += [b, blocks[i % len(blocks)]]
    exp_mixed = [oracle.kv_block_col(b) for b in mixed]
    assert {st for st, _ in exp_mixed} == {0, N.PBL_CORRUPT_BOUNDS, N.PBL_CORRUPT_COLBLK_HEADER}
    for align in (8, 1):
        check_kv(blocks, [oracle.kv_block_col(b) for b in blocks], align, f"shapes, align {align}")
        check_kv(mixed, exp_mixed, align, f"corrupt among good, align {align}")


@functools.lru_cache(maxsize=None)
def kv_pool_expected():
    return tuple(oracle.kv_block_col(b) for b in U.kv_pool()[0])


@pytest.mark.parametrize("n", U.KV_BATCHES)
def test_kv_batches(n):
    check_kv(U.kv_pool()[0][:n], kv_pool_expected()[:n], 1, f"{n} blocks")


def test_kv_capacity():
    cases = U.kv_shape_cases()
    blocks = [c[1] for c in cases]
    counts = [len(c[2]) for c in cases]
    base = np.concatenate([[0], np.cumsum(counts)])
    total = int(base[-1])
    buf, bb = batch_of(blocks)
    for cap in (total, total - 1):
        e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
        out = KvSlices(e(cap, torch.int64), e(cap, torch.int32), e(cap, torch.int64), e(cap, torch.int32),
                       e(len(blocks) + 1, torch.int64), e(len(blocks), torch.int32))
        assert N.lib().pbl_kv_blocks(ctypes.byref(bb.c_struct()), ctypes.byref(out.c_struct()), None) == 0
        torch.cuda.synchronize()
        want = [N.PBL_OVERFLOW if base[i] + counts[i] > cap else 0 for i in range(len(blocks))]
        assert list(out.status()) == want and want.count(N.PBL_OVERFLOW) == (cap < total), cap
        assert np.array_equal(out.blk_base.cpu().numpy(), base), cap
    kv = kv_blocks(bb, cap=3)  # the re-run with the exact size
    assert int(kv.blk_base[len(blocks)].item()) == total and not kv.status().any()


# ---- pbl_valblk_index ------------------------------------------------------------------------------
def valblk_raw(data: bytes, widths, cap=None):
    nw, ow, lw = widths
    w = max(1, nw + ow + lw)
    rows = len(data) // w
    cap = rows if cap is None else cap
    src = torch.from_numpy(np.frombuffer(data + bytes(16), np.uint8).copy()).cuda()
    ho = torch.full((max(rows, 1),), -1, dtype=torch.int64, device="cuda")
    hl = torch.full((max(rows, 1),), -1, dtype=torch.int64, device="cuda")
    n_st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    rc = N.lib().pbl_valblk_index(src.data_ptr(), len(data), nw, ow, lw, ho.data_ptr(), hl.data_ptr(), cap,
                                  n_st.data_ptr(), n_st.data_ptr() + 4, None)
    assert rc == 0
    torch.cuda.synchronize()
    n, st = n_st.cpu().tolist()
    return n, st, ho.cpu().numpy().view(U64), hl.cpu().numpy().view(U64)


def test_valblk_index():
    """Width triples over 1 .. 8 (row widths that are no power of two among
    them), 0 .. 1000 rows, a wrong block number in row 0, in row 256 and in the
    last row, a ragged length, a width of 0 or 9, and a capacity below the row
    count, against valblk.DecodeIndex restated."""
    for name, data, w in U.valblk_cases():
        hs, err = U.decode_valblk_index(data, w)
        n, st, ho, hl = valblk_raw(data, w)
        assert n == len(data) // sum(w), name
        if err:
            assert st == N.PBL_CORRUPT_VALUE_HANDLE, name
            continue
        assert st == 0 and n == len(hs), name
        assert np.array_equal(ho[:n], u64(h[0] for h in hs)) and np.array_equal(hl[:n], u64(h[1] for h in hs)), name
    data = U.valblk_index(U.valblk_handles(10, (2, 3, 2)), (2, 3, 2))
    for w in ((0, 3, 4), (2, 0, 5), (2, 5, 0), (9, 3, 2), (2, 9, 3), (2, 3, 9)):
        n, st, ho, _hl = valblk_raw(data, w)
        assert (n, st) == (0, N.PBL_CORRUPT_VALUE_HANDLE) and ho[0] == U64(U.U64), w
    w = (2, 3, 2)
    hs = U.valblk_handles(300, w)
    n, st, ho, hl = valblk_raw(U.valblk_index(hs, w), w, cap=100)
    assert (n, st) == (300, 0)
    assert np.array_equal(ho[:100], u64(h[0] for h in hs[:100])) and np.array_equal(hl[:100], u64(h[1] for h in hs[:100]))
    assert (ho[100:] == U64(U.U64)).all() and (hl[100:] == U64(U.U64)).all()


# ---- pbl_resolve_values ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_block_batch():
    return BlockBatch.from_blocks(list(U.value_blocks()), "cuda")


SRC = {"row": dict(fmt=N.PBL_FMT_ROW, flags=N.PBL_ROW_VALUE_PREFIX), "col": dict(fmt=N.PBL_FMT_COL_CRDB1, flags=0)}
SRC_ARRAYS = ("trailer", "kv_flags", "key_off", "key_bytes", "blk_kv_base", "blk_key_base")


def expected_resolved(kvs, want_st):
    """(val_off per OK block, blk_val_base, value bytes) from the construction list."""
    vo, base, data = {}, [0], bytearray()
    for b, ks in enumerate(kvs):
        if want_st[b] == 0:
            ends = np.cumsum([0] + [len(k[3]) for k in ks])
            vo[b] = ends
            data += b"".join(k[3] for k in ks)
            base.append(base[-1] + int(ends[-1]))
        else:
            base.append(base[-1])
    return vo, np.array(base, U64), bytes(data)


def check_resolved(src, r, kvs, want_st, ctx):
    """The resolved batch `r` (host) of source `src` (host) against the
    construction list: statuses, status_mask, val_off, blk_val_base, totals and
    bytes; keys, trailers and flags unchanged."""
    vo, base, data = expected_resolved(kvs, want_st)
    assert list(r["blk_status"]) == list(want_st), ctx
    mask = 0
    for st in want_st:
        mask |= (1 << st) if st else 0
    assert r["status_mask"] == mask and r["n_bad_blocks"] == sum(1 for st in want_st if st), ctx
    assert np.array_equal(r["blk_val_base"], base), ctx
    assert r["val_bytes_total"] == len(data) and r["val_bytes"].tobytes() == data, ctx
    kvb = src["blk_kv_base"]
    for b, ends in vo.items():
        k0 = int(kvb[b]) + b
        assert np.array_equal(r["val_off"][k0:k0 + len(ends)], ends.astype(np.uint32)), (ctx, b)
    for k in SRC_ARRAYS:
        assert np.array_equal(r[k], src[k]), (ctx, k)
    assert r["n_kv"] == src["n_kv"] == sum(len(ks) for b, ks in enumerate(kvs) if want_st[b] != 1), ctx


def run_resolve(blocks, fmt):
    d = decode(BlockBatch.from_blocks(list(blocks), "cuda", **SRC[fmt]))
    return d, d.to_host()


@pytest.mark.parametrize("fmt", ["row", "col"])
def test_resolve_block_shapes(fmt):
    """Blocks of 1, 63, 64, 65 and 200 KVs (the wave's running carry), in-place
    and handle values mixed; ValueLen of 1 .. 3 varint bytes, BlockNum of 1 and
    2, OffsetInBlock of 1 .. 3; zero-length values at offset 0 and at the
    block's end; values ending exactly at their block's end."""
    rows, cols, kvs = U.resolve_shape_cases()
    d, src = run_resolve(rows if fmt == "row" else cols, fmt)
    assert src["status_mask"] == 0
    r = resolve_values(d, value_block_batch()).to_host()
    check_resolved(src, r, kvs, [0] * len(kvs), fmt)
    got = [kv.value for b in range(len(kvs)) for kv in kvs_of_block(r, b)]
    assert got == [k[3] for ks in kvs for k in ks]


@pytest.mark.parametrize("fmt", ["row", "col"])
def test_resolve_corrupt_handles(fmt):
    """A value one byte past its block, BlockNum == n_blocks, a handle cut
    after each field, the prefix byte alone, ValueLen >= 2^32:
    PBL_CORRUPT_VALUE_HANDLE for that block alone, which contributes no bytes
    and moves nothing behind it; a block the decode rejected keeps its status.
    Handle varints are Go's 64-bit Uvarint: a field padded to
    six bytes reads as its value, an 11-byte field or a tenth byte above 1 is
    PBL_CORRUPT_VALUE_HANDLE."""
    blocks, kvs, want = U.resolve_corrupt_batch(fmt)
    d, src = run_resolve(blocks, fmt)
    assert list(src["blk_status"]) == [st if st == 1 else 0 for st in want]
    r = resolve_values(d, value_block_batch()).to_host()
    check_resolved(src, r, kvs, want, fmt)


@functools.lru_cache(maxsize=None)
def resolved_pool(fmt):
    blocks, kvs = U.resolve_pool(fmt)
    return blocks, kvs


@pytest.mark.parametrize("fmt,n", [("row", U.SCAN + 1), ("col", U.GRID + 1), ("row", U.WAVE_GRID + 1)])
def test_resolve_batches(fmt, n):
    """1025, 4097 and 16385 tiny blocks over the 131 shared value blocks: a
    second chunk of the scan, a second pass of the write kernel's and of the
    size kernel's grid."""
    blocks, kvs = resolved_pool(fmt)
    blocks, kvs = blocks[:n], kvs[:n]
    d, src = run_resolve(blocks, fmt)
    assert src["status_mask"] == 0
    r = resolve_values(d, value_block_batch()).to_host()
    check_resolved(src, r, kvs, [0] * n, (fmt, n))


def test_resolve_aliasing_overflow_rerun():
    """300 handles naming the same 4 KiB: the resolved bytes exceed
    resolve_values()'s first capacity.  The first pass flags PBL_OVERFLOW on
    exactly the blocks past the capacity and reports the true total; the re-run
    delivers every value."""
    blocks, kvs = U.resolve_alias_case()
    d, src = run_resolve(blocks, "row")
    vb = value_block_batch()
    nb = len(blocks)
    cap = int(d.cap.val) + vb.input_bytes() + 16  # resolve_values()'s first capacity
    per_block = 10 * U.ALIAS_VALUE[0]
    assert cap < nb * per_block
    e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
    vo, vbytes, base, bst = e(d.val_off.numel(), torch.int32), e(cap + 16, torch.uint8), e(nb + 1, torch.int64), \
        e(nb, torch.int32)
    c = N.ValueOutC(vo.data_ptr(), vbytes.data_ptr(), base.data_ptr(), bst.data_ptr(), cap)
    o, v = d.c_struct(), vb.c_struct()
    assert N.lib().pbl_resolve_values(ctypes.byref(o), nb, ctypes.byref(v), ctypes.byref(c), None) == 0
    torch.cuda.synchronize()
    assert list(bst.cpu().numpy()) == [N.PBL_OVERFLOW if (b + 1) * per_block > cap else 0 for b in range(nb)]
    assert base.cpu().tolist() == [b * per_block for b in range(nb + 1)]
    fit = cap // per_block
    assert vbytes[:fit * per_block].cpu().numpy().tobytes() == b"".join(k[3] for ks in kvs[:fit] for k in ks)
    r = resolve_values(d, vb).to_host()
    check_resolved(src, r, kvs, [0] * nb, "alias")


# ---- the whole table ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic():
    data, info = U.synthetic_table(table_bytes("cr_schema_000014.sst"))
    return data, info, Table(data)


def table_kvs(r):
    return [(kv.user_key, kv.trailer, kv.value, kv.flags) for b in range(len(r["blk_status"]))
            for kv in kvs_of_block(r, b)]


def test_table_handles_and_decode():
    """A Pebblev7 table of 4100 data blocks, 1025 lower-level index blocks
    under a top-level block of 1025 rows, and 131 value blocks:
    data_block_handles() equals the handles written, decode() the construction
    list and the oracle's scan, decode(resolve=False) carries the handles."""
    data, info, t = synthetic()
    assert t.two_level() and t.key_schema() == N.PBL_FMT_COL_CRDB1
    h = t.data_block_handles()
    n = int(h.blk_base[-1].item())
    assert h.blk_base.numel() == len(info["lower"]) + 1
    got = list(zip(h.handle_off[:n].cpu().tolist(), h.handle_len[:n].cpu().tolist()))
    assert got == info["data_handles"]
    assert t.value_blocks().n_blocks == info["n_value_blocks"]
    r = t.decode().to_host()
    assert r["status_mask"] == 0
    kvs = table_kvs(r)
    assert [(k, tr, v) for k, tr, v, _fl in kvs] == info["kvs"]
    assert kvs == oracle.table_scan(data)[1]
    raw = table_kvs(t.decode(resolve=False).to_host())
    assert len(raw) == len(info["stored"])
    for (_k, _t, v, fl), (stored, is_handle) in zip(raw, info["stored"]):
        if is_handle:
            assert fl & N.PBL_KV_VALBLK_HANDLE and v[0] & 0xC0 == 0x80 and v[1:] == stored
        else:
            assert not fl & N.PBL_KV_VALBLK_HANDLE and v == stored


def test_table_seek():
    _data, info, t = synthetic()
    keys = [k for k, _t, _v in info["kvs"][::23]]
    keys += [k[:-9] + (int.from_bytes(k[-9:-1], "big") + 1).to_bytes(8, "big") + k[-1:] for k in keys[::3]]
    keys += [b"a\x00", b"k9999999\x00"]  # bare roach keys before the first and behind the last KV
    assert len(keys) > 300
    hst = t.decode(resolve=False).to_host()
    got = device_result(t.seek_ge(keys))
    exp = seek_host(hst, keys, op="ge", comparer=N.PBL_CMP_CRDB)
    assert_seek(got, [x.tolist() for x in exp], "synthetic table")


# ---- physical.hip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [N.PBL_CHECKSUM_CRC32C, N.PBL_CHECKSUM_XXHASH64])
def test_checksums_past_the_grid(kind):
    """16385 blocks of 0 .. 8 bytes: a second pass of the wave-per-block CRC
    grid (physical.hip:488) and far past one pass of the xxhash one."""
    body, off, lens, comp, want = U.checksum_batch(kind)
    st, got = verify_checksums(PhysBatch.from_host(body, off, lens), kind)
    assert np.array_equal(got, comp)
    assert np.array_equal(st, want) and int((want != 0).sum()) == len(want) // U.CORRUPT_EVERY


def test_decompress_past_the_grid():
    """4097 tiny blocks, stored and snappy by turns (physical.hip:515-521)."""
    body, off, lens, exp = U.decompress_batch()
    bb, st = decompress(PhysBatch.from_host(body, off, lens))
    assert not st.any()
    out = bb.blocks.cpu().numpy().tobytes()
    o, n = bb.block_off.cpu().tolist(), bb.block_len.cpu().tolist()
    assert [out[a:a + m] for a, m in zip(o, n)] == list(exp)
