"""The snapshot-visible view on the device (pbl_visible_size / pbl_visible_batch,
pebble_amd/csrc/visible.hip) over batches decoded on the device.  The expected
result is the host's over to_host() of the same batch (pbl_visible_batch_host,
the sequential state machine; every array and total compared exactly), the
Python statement of the rules (visibleutil.expected_visible) and the
reference's own iterator test data (tests/golden/iterator_points.json)."""
import ctypes

import numpy as np
import pytest

from pebble_amd import _native as N
from pebble_amd.rowblk import Writer
from pebble_amd.visible import read, visible, visible_host
from scanutil import ARRAYS, result_kvs
from visibleutil import (D, MAX, assert_same, assert_visible_is, cases, device_result, expected_visible, fold, golden_block,
                         load_golden, one_key_block, replay)

pytestmark = pytest.mark.gpu

CASES = cases()


def dev_decode(blocks):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0))


def row_block(kvs, restart=4):
    w = Writer(restart)
    for kv in kvs:
        w.add(kv[0], kv[1], kv[2])
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def dev_batch(blocks, restart=4):
    """The case's blocks as row blocks, decoded on the device; a KV's fourth
    element is OR-ed into its kv_flags (a row block cannot say "handle" without
    a value block to point into)."""
    import torch
    d = dev_decode([corrupt(row_block([(b"x", 1 << 8 | 1, b"")])) if b is None else row_block(b, restart) for b in blocks])
    extra = [kv[3] if len(kv) > 3 else 0 for b in blocks for kv in (b or [])]
    if any(extra):
        d.kv_flags[: len(extra)] |= torch.tensor(extra, dtype=torch.uint8, device="cuda")
    return d


def check(d, comparer, snapshot, keep, ctx="", python=True):
    """Device against pbl_visible_batch_host (every array and total) and against
    the Python model.  Returns (device result, the input's host arrays)."""
    h = d.to_host()
    r = device_result(visible(d, comparer=comparer, snapshot=snapshot, keep_operands=keep))
    assert_same(r, visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep), ctx)
    if python:
        assert_visible_is(r, h, comparer, snapshot, keep, ctx)
    return r, h


# ---- 1. the hand-built cases: device against host and against Python ----------------------------
@pytest.mark.parametrize("name,comparer,blocks,snaps", CASES, ids=[c[0] for c in CASES])
def test_hand_built_cases(name, comparer, blocks, snaps):
    if not blocks:  # a batch with no blocks at all
        from pebble_amd.batch import Capacity, DecodedBatch
        d = DecodedBatch.allocate(0, Capacity(0, 0, 0, 0), "cuda", restarts=False)
        d.blk_kv_base.zero_(), d.blk_key_base.zero_(), d.blk_val_base.zero_(), d.totals.zero_()
    else:
        d = dev_batch(blocks, restart=(1, 4, 16)[len(name) % 3])
    h = d.to_host()
    assert [int(s != 0) for s in h["blk_status"]] == [int(b is None) for b in blocks], name
    assert h["n_kv"] == sum(len(b) for b in blocks if b is not None), name
    for s in snaps:
        got = {}
        for keep in (False, True):
            got[keep], _ = check(d, comparer, s, keep, (name, s, keep))
        # folding the kept operands reproduces the default mode's values
        for q in range(len(blocks)):
            if int(got[False][0]["blk_status"][q]) == 0:
                kept = [kv + (int(x), int(n)) for kv, x, n in zip(
                    result_kvs(got[True][0], q), got[True][1][int(got[True][0]["blk_kv_base"][q]):],
                    got[True][2][int(got[True][0]["blk_kv_base"][q]):])]
                assert [x[:3] for x in fold(kept)] == [x[:3] for x in result_kvs(got[False][0], q)], (name, s, q)
        if s == 0:
            assert got[False][0]["n_kv"] == 0 and got[False][0]["status_mask"] == 0, name


# ---- 2. one user key across the cross-tile scan boundary ----------------------------------------
def test_one_key_with_70000_versions():
    d = dev_batch([one_key_block()], restart=16)
    for snapshot, n in ((MAX, 70000), (35001, 35000)):
        (r, src_kv, n_src), h = check(d, D, snapshot, False, snapshot, python=False)
        assert h["n_kv"] == 70000
        (k, t, v, f), = result_kvs(r, 0)
        assert (k, t >> 8, t & 0xff) == (b"the key", n, 2) and n_src.tolist() == [n] and src_kv.tolist() == [70000 - n]
        assert v == bytes(s % 251 for s in range(1, n + 1))
        (r, src_kv, n_src), _ = check(d, D, snapshot, True, snapshot, python=False)
        assert r["n_kv"] == n and n_src[:3].tolist() == [n, 0, 0] and not n_src[1:].any()
        assert src_kv.tolist() == list(range(70000 - n, 70000))


# ---- 3. the reference's iterator test data -------------------------------------------------------
def test_golden_iterator_cases():
    g = load_golden()
    assert len(g["cases"]) >= 45 and sum(len(c["expected"]) for c in g["cases"]) >= 102
    lines = 0
    for seq in sorted({c["seq"] for c in g["cases"]}):  # one batch per snapshot, a block per case
        mine = [c for c in g["cases"] if c["seq"] == seq]
        d = dev_batch([golden_block(c, g["kinds"]) for c in mine])
        r = visible(d, comparer=D, snapshot=seq).batch.to_host()
        assert r["status_mask"] == 0
        for q, c in enumerate(mine):
            kvs = [(k, v) for k, _, v, _ in result_kvs(r, q)]
            assert replay(kvs, c["commands"]) == c["expected"], (seq, q, c)
            lines += len(c["expected"])
    assert lines >= 102


# ---- 4. chaining: read() over tables, and the result as a decoded batch --------------------------
class BlocksTable:
    """What merge_scan needs of a table, over row blocks decoded on the device."""

    def __init__(self, kvs, per_block, restart):
        self.d = dev_decode([row_block(kvs[i:i + per_block], restart) for i in range(0, len(kvs), per_block)])

    def comparer(self):
        return D

    def scan(self, lowers, uppers, hide_obsolete_points=False):
        from pebble_amd.scan import scan
        return scan(self.d, lowers, uppers, comparer=D, hide_obsolete_points=hide_obsolete_points)


def test_read_over_three_tables():
    from pebble_amd.merge import merge_host
    from pebble_amd.scan import scan, scan_host
    from pebble_amd.seek import seek, seek_host
    from visibleutil import DEL, MERGE, SET, tr
    kinds = [SET, MERGE, DEL, MERGE, MERGE, SET, MERGE, SET, DEL]
    kvs = [(b"u%04d" % (i // 5), tr(3000 - i, kinds[(i * 7 + i // 5) % 9]), b"val%d;" % i * (1 + i % 4)) for i in range(1500)]
    tables = [BlocksTable(kvs[r::3], (130, 256, 77)[r], (1, 4, 16)[r]) for r in range(3)]
    lo, up = [None, b"u0100", b"u0250"], [None, b"u0200", b"u0250\x00"]
    for snapshot in (MAX, 2200):
        res = read(tables, lo, up, snapshot=snapshot)
        r = device_result(res)
        # the union of the tables' KVs per range, merged on the host, under the Python model
        hosts = [t.scan(lo, up).batch.to_host() for t in tables]
        union = merge_host(hosts, comparer=D)[0]
        exp = assert_visible_is(r, union, D, snapshot, False, snapshot)
        assert len(exp[0][1]) > 100 and 0 < len(exp[1][1]) < len(exp[0][1]) and len(exp[2][1]) <= 1
    # the result is a decoded batch: a per-block seek and a scan read it
    h = r[0]
    keys = [b"u0000", b"u0150", b"u0150\x00", b"zz"]
    got = seek(res.batch, keys, op="ge", comparer=D, blocks=[0, 1, 1, 0])
    want = seek_host(h, keys, op="ge", comparer=D, blocks=[0, 1, 1, 0])
    assert got.kv.cpu().numpy().view(np.uint64).tolist() == want[0].tolist()
    sr = scan(res.batch, [b"u0170"], [b"u0180"], comparer=D, blocks=[1]).batch.to_host()
    se = scan_host(h, [b"u0170"], [b"u0180"], comparer=D, blocks=[1])[0]
    assert sr["n_kv"] == se["n_kv"] > 0
    for k in ARRAYS:
        assert (np.asarray(sr[k]).astype(np.uint64) == np.asarray(se[k]).astype(np.uint64)).all(), k


def test_read_on_real_tables():
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    data = table_bytes("h_no_compression.sst")
    t0, t1 = Table(data), Table(data)
    one = t0.scan([None], [None]).batch.to_host()
    got, src_kv, n_src = device_result(read([t0, t1], [None], [None]))
    assert got["status_mask"] == 0
    exp = expected_visible(one, t0.comparer())[0][1]
    assert [x[:3] for x in result_kvs(got, 0)] == [x[:3] for x in exp] and len(exp) > 0
    assert src_kv.tolist() == [2 * x[4] for x in exp]  # every KV twice in the merge; the first of a pair is the head


def test_meta_and_entry_offsets_travel_with_the_head():
    import torch
    _, comparer, blocks, _ = next(c for c in CASES if c[0] == "wave and tile edges")
    d = dev_batch(blocks)
    n = d.to_host()["n_kv"]
    d.tiering_span_id = torch.arange(n, dtype=torch.int64, device="cuda") + 1000
    d.tiering_attr = torch.arange(n, dtype=torch.int64, device="cuda") * 3
    for keep in (False, True):
        (r, src_kv, _), h = check(d, comparer, 2500, keep, ("meta", keep))
        at = src_kv.astype(np.int64)
        assert r["n_kv"] > 0
        for k in ("entry_off", "tiering_span_id", "tiering_attr", "trailer"):
            assert (r[k] == h[k][at]).all(), (k, keep)


# ---- 5. overflow, and a call without a size pass --------------------------------------------------
def test_overflow_writes_sizes_and_nothing_else():
    import torch
    from pebble_amd.batch import Capacity, DecodedBatch
    _, comparer, blocks, _ = next(c for c in CASES if c[0] == "wave and tile edges")
    d = dev_batch(blocks)
    h = d.to_host()
    full = visible_host(h, comparer=comparer)
    caps = (full[0]["n_kv"], full[0]["key_bytes_total"], full[0]["val_bytes_total"])
    nb, n_kv = d.n_blocks, h["n_kv"]
    vin = N.VisibleInC(d.c_struct(), nb, comparer, n_kv, MAX)
    ws = torch.empty(int(N.lib().pbl_visible_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device="cuda")
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        out = DecodedBatch.allocate(nb, Capacity(cap[0], cap[1], cap[2], 0), "cuda", restarts=False)
        bufs = (out.trailer, out.kv_flags, out.entry_off, out.key_off, out.val_off, out.key_bytes, out.val_bytes)
        for x in bufs:
            x.view(torch.uint8).fill_(0xAA)
        sk = torch.full((caps[0],), -1, dtype=torch.int64, device="cuda")
        ns = torch.full((caps[0],), -1, dtype=torch.int32, device="cuda")
        vo = N.VisibleOutC(out.c_struct(), sk.data_ptr(), ns.data_ptr())
        rc = N.lib().pbl_visible_batch(ctypes.byref(vin), ctypes.byref(vo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0,
                                       None)
        assert rc == N.PBL_OK
        torch.cuda.synchronize()
        t = out.read_totals()
        assert t.status_mask == 1 << N.PBL_OVERFLOW and (t.n_kv, t.key_bytes, t.val_bytes) == caps, short
        for k in ("blk_kv_base", "blk_key_base", "blk_val_base"):
            assert getattr(out, k).cpu().numpy().view(np.uint64).tolist() == full[0][k].tolist(), (short, k)
        assert out.blk_status.cpu().tolist() == [0] * nb
        for x in bufs:
            assert bool((x.view(torch.uint8) == 0xAA).all()), short
        assert bool((sk == -1).all()) and bool((ns == -1).all())
    # the same workspace, enough room, in one call (no size pass before it)
    out = DecodedBatch.allocate(nb, Capacity(caps[0], caps[1], caps[2], 0), "cuda", entry_off=False, restarts=False)
    sk = torch.empty(caps[0], dtype=torch.int64, device="cuda")
    ns = torch.empty(caps[0], dtype=torch.int32, device="cuda")
    vo = N.VisibleOutC(out.c_struct(), sk.data_ptr(), ns.data_ptr())
    assert N.lib().pbl_visible_batch(ctypes.byref(vin), ctypes.byref(vo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0,
                                     None) == N.PBL_OK
    torch.cuda.synchronize()
    h2 = dict(h, entry_off=None)
    assert_same((out.to_host(), sk.cpu().numpy().view(np.uint64), ns.cpu().numpy().view(np.uint32)),
                visible_host(h2, comparer=comparer), "one call")
