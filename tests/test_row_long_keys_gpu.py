"""Row keys longer than the general walk's 32 KiB LDS key buffer on the device
(ABI v9: the key continues in a spill slot of the workspace,
pbl_workspace_bytes_for) against the CPU oracle, which like Go's readEntry
grows the key without bound: bit-exact on every output array.

Long-key blocks of 33-205 KiB (tests/longkeyutil.py: the shapes a-g at restart
intervals 1, 2 and 16) sit between ordinary 32 KiB blocks.  Every flag set is
decoded on the staging-pool kernel (PBL_KERNEL_POOL), in the two-pass form
(PBL_BATCH_VARLEN; value prefixes and HideObsoletePoints need key bytes to
size a block and take the pool kernel there too) and under the default
routing; one batch interleaves crdb1 colblk blocks.  Without the spill slots
(a workspace of pbl_workspace_bytes) such a block is PBL_UNSUPPORTED and every
other block is unaffected, which is what every long-key block reported before
ABI v9."""
import functools

import numpy as np
import pytest

import oracle
from longkeyutil import C, corrupt_blocks, long_key_blocks, raw_row_block, shape_a, slot_loop_blocks
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode, decode_into, size_batch
from pebble_amd.rowblk import gen_row_blocks
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
G = N.PBL_LONGKEY_WGS
SEQ = 4242
FLAGSETS = {"plain": 0, "raw": N.PBL_ROW_RAW_KEYS, "vprefix": N.PBL_ROW_VALUE_PREFIX, "hide": N.PBL_ROW_HIDE_OBSOLETE,
            "seq": 0}
ROUTES = {"pool": N.PBL_KERNEL_POOL, "varlen": N.PBL_BATCH_VARLEN, "default": 0}


@functools.lru_cache(maxsize=None)
def ordinary(n=10):
    buf, off, lens, _ = gen_row_blocks(17, n, 32768, 16, 16, 100)
    return [bytes(buf[int(o): int(o) + int(ln)]) for o, ln in zip(off, lens)]


@functools.lru_cache(maxsize=None)
def batch(ri):
    """The long-key and corrupt blocks of restart interval ri spread among ten
    ordinary blocks (two long-key blocks in a row too); (buf, off, lens, names)."""
    named = long_key_blocks(ri) + corrupt_blocks(ri)
    rows = ordinary()
    blocks, names = [], []
    for i, (name, blk) in enumerate(named):
        if i % 2 == 0:
            blocks.append(rows[(i // 2) % len(rows)])
            names.append("ordinary")
        blocks.append(blk)
        names.append(name)
    blocks.append(rows[-1])
    names.append("ordinary")
    return pack(blocks) + (names,)


@functools.lru_cache(maxsize=None)
def reference(ri, fs):
    buf, off, lens, _ = batch(ri)
    flags = FLAGSETS[fs]
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, None, flags)
    if fs == "seq":
        o = oracle.transform_batch(o, SEQ, False, b"", b"", 0, src=(buf, off, lens, N.PBL_FMT_ROW, None, flags))
    return o


def gpu(buf, off, lens, flags, seq=0, cap=None, block_format=None):
    bb = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags, block_format=block_format)
    bb.synthetic_seq_num = seq
    assert bb.max_block_len == int(max(lens))
    return bb, decode(bb, cap=cap)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("fs", list(FLAGSETS))
@pytest.mark.parametrize("ri", [1, 2, 16])
def test_long_key_blocks_match_the_oracle(ri, fs, route):
    buf, off, lens, names = batch(ri)
    o = reference(ri, fs)
    long_ok = [i for i, n in enumerate(names) if n != "ordinary" and n[0] not in "fg"]
    assert all(o["blk_status"][i] == N.PBL_OK for i in long_ok)  # (the oracle decodes them: not vacuous)
    bad = [i for i, n in enumerate(names) if n[0] in "fg" and n != "ordinary"]
    assert bad and all(o["blk_status"][i] == N.PBL_CORRUPT_BOUNDS for i in bad)
    _, d = gpu(buf, off, lens, FLAGSETS[fs] | ROUTES[route], SEQ if fs == "seq" else 0)
    g = d.to_host()
    for i in long_ok:
        assert g["blk_status"][i] == N.PBL_OK, f"{names[i]}: device status {g['blk_status'][i]}"
    assert_same(g, o, f"ri={ri} {fs} {route}")
    assert g["n_slow_blocks"] >= len(long_ok)


def test_mixed_batch_with_colblk_blocks():
    from pebble_amd.colblk import gen_col_blocks
    buf, off, lens, names = batch(2)
    rows = [bytes(buf[int(o): int(o) + int(ln)]) for o, ln in zip(off, lens)]
    cb, co, cl, _ = gen_col_blocks(5, len(rows), 8192)
    cols = [bytes(cb[co[i]:co[i] + cl[i]]) for i in range(len(rows))]
    blocks = [x for p in zip(rows, cols) for x in p]
    bf = np.array([N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1] * len(rows), np.uint8)
    mbuf, moff, mlens = pack(blocks)
    for flags in (0, N.PBL_ROW_HIDE_OBSOLETE):
        o = oracle.decode_batch(mbuf, moff, mlens, N.PBL_FMT_ROW, bf, flags)
        bb, d = gpu(mbuf, moff, mlens, flags, block_format=bf)
        assert_same(d.to_host(), o, f"mixed flags={flags}")
        t = size_batch(bb).read_totals()
        assert (t.n_kv, t.key_bytes, t.val_bytes, t.status_mask) == \
            (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["status_mask"])


@pytest.mark.parametrize("route", list(ROUTES))
def test_more_long_key_blocks_than_slots(route):
    """G + 3 blocks of 41 KiB: every workgroup's loop over the list, slots reused."""
    blocks = slot_loop_blocks(G + 3)
    rows = ordinary()
    blocks = blocks[:5] + [rows[0]] + blocks[5:20] + [rows[1]] + blocks[20:]
    buf, off, lens = pack(blocks)
    o = oracle.rowblk_decode_batch(buf, off, lens, 0)
    assert o["status_mask"] == 0
    _, d = gpu(buf, off, lens, ROUTES[route])
    assert_same(d.to_host(), o, f"G+3 {route}")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("fs", ["plain", "hide"])
def test_size_pass_and_overflow(fs, route):
    """size_batch gives the decode's bases and totals; capacities of 10 give
    PBL_OVERFLOW with exact sizes, and the retry decodes."""
    import torch
    buf, off, lens, names = batch(2)
    flags = FLAGSETS[fs] | ROUTES[route]
    o = reference(2, fs)
    bb = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags)
    s = size_batch(bb)
    torch.cuda.synchronize()
    ts = s.read_totals()
    assert (ts.n_kv, ts.key_bytes, ts.val_bytes, ts.n_restarts, ts.status_mask, ts.n_bad_blocks) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"], o["status_mask"], o["n_bad_blocks"])
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base"):
        assert np.array_equal(getattr(s, k).cpu().numpy().view(np.uint64), o[k]), k
    assert np.array_equal(s.blk_status.cpu().numpy().view(np.uint32), o["blk_status"])
    out = DecodedBatch.allocate(bb.n_blocks, Capacity(kv=10, key=10, val=10, rst=10), "cuda",
                                max_block_len=bb.max_block_len)
    decode_into(bb, out)
    torch.cuda.synchronize()
    t = out.read_totals()
    assert t.status_mask & (1 << N.PBL_OVERFLOW)
    assert (t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"])
    st = out.blk_status.cpu().numpy().view(np.uint32)
    assert not (st == N.PBL_UNSUPPORTED).any()
    h = decode(bb, cap=Capacity(kv=10, key=10, val=10, rst=10)).to_host()
    assert_same(h, o, f"retry {fs} {route}")


def _without(o, drop):
    """The oracle's batch with the blocks `drop` reporting PBL_UNSUPPORTED and
    no outputs (what a failed block leaves: a zero aggregate)."""
    buf, off, lens = o
    blocks = [bytes(buf[int(a): int(a) + int(n)]) for a, n in zip(off, lens)]
    # a block that fails Iter.Init (no restarts) has the same zero aggregate
    for i in drop:
        blocks[i] = b"\x00" * 8
    r = oracle.rowblk_decode_batch(*pack(blocks), 0)
    for i in drop:
        assert r["blk_status"][i] == N.PBL_CORRUPT_NO_RESTARTS
        r["blk_status"][i] = N.PBL_UNSUPPORTED
    r["status_mask"] = (r["status_mask"] & ~(1 << N.PBL_CORRUPT_NO_RESTARTS)) | (1 << N.PBL_UNSUPPORTED)
    return r


@pytest.mark.parametrize("route", list(ROUTES))
def test_workspace_without_slots_keeps_the_old_result(route):
    """max_block_len = 0 (the workspace of pbl_workspace_bytes): the long-key
    blocks report PBL_UNSUPPORTED, every other block equals the oracle."""
    import torch
    buf, off, lens, names = batch(16)
    o = reference(16, "plain")
    bb = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, ROUTES[route])
    t = size_batch(bb).read_totals()
    cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), int(t.n_restarts))
    out = DecodedBatch.allocate(bb.n_blocks, cap, "cuda", max_block_len=0)
    assert out.workspace.numel() == N.lib().pbl_workspace_bytes(bb.n_blocks)
    decode_into(bb, out)
    torch.cuda.synchronize()
    g = out.to_host()
    # which blocks hold a key past the buffer: all long-key blocks but the one
    # whose longest key is C; the corrupt blocks too (their first key is long:
    # the walk stops there, before the corrupt entry)
    drop = [i for i, n in enumerate(names) if n != "ordinary" and n != f"a klen={C}"]
    assert len(drop) >= 17
    assert_same(g, _without((buf, off, lens), drop), f"no slots {route}")
    keep = [i for i in range(len(names)) if i not in drop]
    assert all(g["blk_status"][i] == o["blk_status"][i] for i in keep)


def test_a_key_that_outgrows_its_slot():
    """A workspace sized for 48 KiB blocks: a block with a 100 KiB key is
    PBL_UNSUPPORTED, a 40 KiB key in the same batch decodes."""
    import torch
    rows = ordinary()
    k40 = raw_row_block(shape_a(40 * 1024), 16)
    k100 = raw_row_block(shape_a(100 * 1024)[:3], 16)
    blocks = [rows[0], k40, rows[1], k100, rows[2], k40]
    buf, off, lens = pack(blocks)
    for route in ROUTES.values():
        bb = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, route)
        full = decode(bb).to_host()
        assert_same(full, oracle.rowblk_decode_batch(buf, off, lens, 0), "full slots")
        cap = Capacity(full["n_kv"], full["key_bytes_total"], full["val_bytes_total"], full["n_restarts"])
        out = DecodedBatch.allocate(bb.n_blocks, cap, "cuda", max_block_len=48 * 1024)
        decode_into(bb, out)
        torch.cuda.synchronize()
        assert_same(out.to_host(), _without((buf, off, lens), [3]), f"48 KiB slots route={route}")
