"""Batched bounded scans on the device (pbl_scan_prepare / pbl_scan_size /
pbl_scan_batch, pebble_amd/csrc/scan.hip) over batches decoded on the device.
The expected result is always the host's over to_host() of the same decoded
batch: pbl_scan_batch_host for whole query sets, every array compared exactly
(scanutil.assert_same), and on the hand-built cases also the walk of the
one-key iterator (scanutil.expected_scan), with each result re-read through
DataIter."""
import ctypes
import dataclasses
import random

import numpy as np
import pytest

from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, gen_row_blocks, make_trailer
from pebble_amd.scan import pack_bounds, prepare, scan, scan_host
from scanutil import assert_same, assert_scan_is, device_result, expected_scan, result_kvs
from seekutil import block_keys, trailer_index

pytestmark = pytest.mark.gpu

D, T, C = N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB


def dev_decode(blocks, fmt=N.PBL_FMT_ROW, block_format=None, flags=0):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", fmt, flags, block_format=block_format))


def row_block(keys, seq0, obsolete=None, restart=4, values=None):
    w = Writer(restart)
    for i, k in enumerate(keys):
        v = values[i] if values is not None else b"v%d" % i
        w.add_with_optional_value_prefix(k, make_trailer(seq0 + i, 1), bool(obsolete and obsolete[i]), v,
                                         len(k), False, 0, False)
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def check(d, h, lo, up, comparer, blocks=None, hide=False, index=None, walk=False, tidx=None, ctx=""):
    """Device against pbl_scan_batch_host (every array) and, with `walk`, both
    against the iterator walk; returns the device result."""
    r = device_result(scan(d, lo, up, comparer=comparer, blocks=blocks, hide_obsolete_points=hide, index=index))
    e = scan_host(h, lo, up, comparer=comparer, blocks=blocks, hide_obsolete_points=hide)
    assert_same(r, e, (ctx, hide))
    if walk:
        exp = expected_scan(h, lo, up, comparer, blocks, hide, tidx)
        assert_scan_is(e, exp, comparer, (ctx, hide, "host"))
        assert_scan_is(r, exp, comparer, (ctx, hide, "device"))
    return r


def all_keys(h):
    return [k for b in range(len(h["blk_status"])) if int(h["blk_status"][b]) == 0 for k in block_keys(h, b)]


# ---- 1. tile and wave edges -------------------------------------------------------------
def test_tile_and_wave_edges():
    keys = [b"k%05d" % i for i in range(1200)]
    blocks = [row_block(keys[i:i + 300], 1 + i) for i in range(0, 1200, 300)]
    d = dev_decode(blocks)
    h = d.to_host()
    assert h["status_mask"] == 0 and h["n_kv"] == 1200
    lo, up = [], []
    for start in (0, 256, 512, 1, 255, 257, 300, 687):  # tile-aligned and not
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 513):
            lo.append(keys[start])
            up.append(keys[start + n] if start + n < 1200 else None)
    idx = prepare(d, D, False, len(lo))
    tidx = trailer_index(h)
    for n in (1, 63, 65):  # partial waves of queries
        check(d, h, lo[-n:], up[-n:], D, index=idx, ctx=("edges", n))
    r = check(d, h, lo, up, D, index=idx, walk=True, tidx=tidx, ctx="edges all")
    sizes = np.diff(r[0]["blk_kv_base"]).tolist()
    assert sizes[:9] == [0, 1, 63, 64, 65, 255, 256, 257, 513] and sizes[9:18] == sizes[:9]
    assert r[1][9].tolist() == [256, 256] and r[1][17].tolist() == [256, 769]
    assert sizes[-1] == 1200 - 687  # [k00687, +inf)


# ---- 2. block boundaries -------------------------------------------------------------------
def test_block_boundaries_and_a_corrupt_block():
    rng = random.Random(5)
    sizes = [3, 40, 7, 5, 17, 3, 29]
    keys, blocks = [], []
    for i, n in enumerate(sizes):
        ks = [b"b%02d_%03d" % (i, j) for j in range(n)]
        keys.append(ks)
        blocks.append(row_block(ks, 1000 * i + 1, restart=rng.choice([1, 4, 16])))
    blocks[3] = corrupt(blocks[3])
    d = dev_decode(blocks)
    h = d.to_host()
    nb = len(blocks)
    assert int(h["blk_status"][3]) != 0 and int(h["blk_kv_base"][4]) == int(h["blk_kv_base"][3])
    tidx = trailer_index(h)
    pts = [None] + [k for ks in keys for k in (ks[0], ks[1], ks[-1], ks[-1] + b"\x00")]
    lo = [a for a in pts for _ in pts]
    up = [b for _ in pts for b in pts]
    r = check(d, h, lo, up, D, walk=True, tidx=tidx, ctx="boundaries")
    assert r[0]["status_mask"] == 0
    # the corrupt block's neighbours join up
    r = check(d, h, [keys[2][-1]], [keys[4][0] + b"\x00"], D, walk=True, tidx=tidx, ctx="across")
    assert [k for k, _, _, _ in result_kvs(r[0], 0)] == [keys[2][-1], keys[4][0]]
    assert r[2].tolist() == [int(h["blk_kv_base"][3]) - 1, int(h["blk_kv_base"][3])]
    # per-block mode: every block, the corrupt one, one past n_blocks
    for b in range(nb + 1):
        lo = [None, keys[min(b, nb - 1)][1], keys[0][0], b"z"]
        up = [None, keys[min(b, nb - 1)][-1], None, None]
        r = check(d, h, lo, up, D, blocks=[b] * 4, walk=True, tidx=tidx, ctx=("block", b))
        st = r[0]["blk_status"].tolist()
        if b == 3:
            assert st == [int(h["blk_status"][3])] * 4 and r[0]["n_kv"] == 0 and r[0]["n_bad_blocks"] == 4
        elif b == nb:
            assert st == [N.PBL_INVALID_ARG] * 4 and r[0]["status_mask"] == 1 << N.PBL_INVALID_ARG
        else:
            assert st == [0] * 4 and np.diff(r[0]["blk_kv_base"]).tolist()[0] == sizes[b]


# ---- 3. HideObsoletePoints ---------------------------------------------------------------
def test_hidden_runs_cross_blocks():
    b0, b1, b2 = [b"a1", b"a2", b"a3", b"a4"], [b"b1", b"b2", b"b3"], [b"c1", b"c2", b"c3"]
    blocks = [row_block(b0, 1, [0, 0, 1, 1]), row_block(b1, 100, [1, 1, 1]), row_block(b2, 200, [1, 0, 0])]
    d = dev_decode(blocks)
    h = d.to_host()
    tidx = trailer_index(h)
    pts = [None] + b0 + b1 + b2 + [b"d"]
    lo = [a for a in pts for _ in pts]
    up = [b for _ in pts for b in pts]
    for hide in (False, True):
        check(d, h, lo, up, D, hide=hide, walk=True, tidx=tidx, ctx="hidden table")
        for b in range(3):
            check(d, h, lo, up, D, blocks=[b] * len(lo), hide=hide, walk=True, tidx=tidx, ctx=("hidden block", b))
    r = device_result(scan(d, [b"a2", b"a3", None], [b"c3", b"c2", None], comparer=D, hide_obsolete_points=True))
    assert r[2].tolist() == [1, 8, 0, 1, 8, 9] and r[1].tolist() == [[1, 9], [2, 8], [0, 10]]  # [a3, c2): all hidden
    r = device_result(scan(d, [None], [None], comparer=D, blocks=[1], hide_obsolete_points=True))
    assert r[0]["n_kv"] == 0 and r[0]["blk_status"].tolist() == [0]  # a block that is entirely obsolete


def test_hidden_runs_cross_tile_edges():
    keys = [b"h%05d" % i for i in range(700)]
    obs = [250 <= i < 263 or 500 <= i < 530 or i % 7 == 3 for i in range(700)]
    blocks = [row_block(keys[:300], 1, obs[:300]), row_block(keys[300:600], 301, obs[300:600]),
              row_block(keys[600:], 601, obs[600:])]
    d = dev_decode(blocks)
    h = d.to_host()
    tidx = trailer_index(h)
    starts = [0, 249, 250, 255, 256, 257, 262, 263, 499, 511, 512, 513, 529, 530]
    lo = [keys[a] for a in starts for _ in starts]
    up = [keys[b] for _ in starts for b in starts]
    check(d, h, lo + [None], up + [None], D, hide=True, walk=True, tidx=tidx, ctx="tile edge hide")
    check(d, h, lo + [None], up + [None], D, hide=False, ctx="tile edge")


def test_hidden_generated_rows():
    rng = random.Random(31)
    buf, off, lens, _ = gen_row_blocks(9, 16, 32768, 16, 16, 100, n_threads=4, obsolete_every=3)
    d = dev_decode([bytes(buf[int(o): int(o) + int(n)]) for o, n in zip(off, lens)])
    h = d.to_host()
    assert (h["kv_flags"] & N.PBL_KV_OBSOLETE).any()
    keys = all_keys(h)
    n = len(keys)
    lo, up = [], []
    for _ in range(300):
        a = rng.randrange(n)
        ln = rng.choice([0, 1, 2, 16, 64, 270, 271, 272, 600])
        lo.append(rng.choice([keys[a], keys[a][:-1], keys[a] + b"\x01"]))
        up.append(keys[a + ln] if a + ln < n else None)
    for hide in (True, False):
        idx = prepare(d, D, hide, len(lo))
        check(d, h, lo, up, D, hide=hide, index=idx, ctx="gen obs table")
        blk = [rng.randrange(16) for _ in lo]
        check(d, h, lo, up, D, blocks=blk, hide=hide, index=idx, ctx="gen obs block")
    check(d, h, lo[:12], up[:12], D, hide=True, walk=True, ctx="gen obs walk")


# ---- 4. copy paths ------------------------------------------------------------------------
def test_copy_paths():
    """Key and value lengths around every branch of the emit's copies (16-B
    chunks, the 64-B unrolled step, values of at most / more than 512 B), and
    results that begin at every byte residue mod 16."""
    klens = [15, 16, 17, 31, 33, 63, 64, 65, 129]
    vlens = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 512, 513, 1025]
    keys, vals = [], []
    for j in range(20):  # one-byte keys and values: every residue at the start of a range
        keys.append(bytes([1 + j]))
        vals.append(bytes([0x80 + j]))
    i = 0
    for kl in klens:
        for vl in vlens:
            keys.append((b"m%04d" % i + b"x" * 200)[:kl])
            vals.append(bytes((i + t) & 0xff for t in range(vl)))
            i += 1
    order = sorted(set(keys))
    assert len(order) == len(keys)
    kv = dict(zip(keys, vals))
    blocks = [row_block(order[:37], 1, values=[kv[k] for k in order[:37]]),
              row_block(order[37:], 1000, values=[kv[k] for k in order[37:]])]
    d = dev_decode(blocks)
    h = d.to_host()
    assert h["status_mask"] == 0
    n = len(order)
    lo, up = [], []
    for a in range(n):
        for ln in (1, 2):  # 3 bytes per pair of one-byte KVs: every residue mod 16 comes up
            lo.append(order[a])
            up.append(order[a + ln] if a + ln < n else None)
    lo.append(None)
    up.append(None)
    r = check(d, h, lo, up, D, walk=True, ctx="copy paths")
    nq = len(lo)
    assert set((r[0]["blk_key_base"][:nq] % 16).tolist()) == set(range(16))
    assert set((r[0]["blk_val_base"][:nq] % 16).tolist()) == set(range(16))
    src_key = h["blk_key_base"][0] + h["key_off"][:20].astype(np.uint64)
    assert set((src_key % 16).tolist()) == set(range(16))
    got = {k: v for k, _, v, _ in result_kvs(r[0], nq - 1)}
    assert got == kv


# ---- 5. comparers ---------------------------------------------------------------------------
def test_testkeys_suffix_order():
    from pebble_amd.colblk import SCHEMA_DEFAULT, DataBlockEncoder
    P = b"c_prefix_longer_than_sixteen_bytes_"
    b0 = [b"a", b"a@10", b"a@3", b"b@5", b"b@5_synthetic"]
    b1 = [P + b"a@9", P + b"a@2", P + b"b", P + b"b@100", P + b"b@20"]
    blocks, seq = [], 1
    for ks in (b0, b1):
        w = DataBlockEncoder(SCHEMA_DEFAULT, 16)
        for k in ks:
            w.add(k, make_trailer(seq, 1), b"v" + k)
            seq += 1
        blocks.append(w.finish())
    d = dev_decode(blocks, N.PBL_FMT_COL_DEFAULT)
    h = d.to_host()
    assert h["status_mask"] == 0 and block_keys(h, 0) == b0 and block_keys(h, 1) == b1
    tidx = trailer_index(h)
    pts = [None, b"a", b"a@10", b"a@7", b"a@3", b"a@1", b"b", b"b@5", b"b@5_synthetic", b"b@4", b"c",
           P + b"a", P + b"a@9", P + b"a@5", P + b"b@50", P + b"b@1", P + b"c", P[:16]]
    lo = [a for a in pts for _ in pts]
    up = [b for _ in pts for b in pts]
    check(d, h, lo, up, T, walk=True, tidx=tidx, ctx="tk table")
    for b in (0, 1):
        check(d, h, lo, up, T, blocks=[b] * len(lo), walk=True, tidx=tidx, ctx=("tk block", b))
    r = device_result(scan(d, [b"a@10", b"a", b"b@5", b"a@3"], [b"a@3", b"b", b"b@5_synthetic", b"a@10"],
                           comparer=T))
    # "@10" sorts before "@3"; "@5_synthetic" compares equal to "@5"; [a@3, a@10) is inverted
    assert r[2].tolist() == [1] + [0, 1, 2] and np.diff(r[0]["blk_kv_base"]).tolist() == [1, 3, 0, 0]


def test_crdb_reference_table():
    from pebble_amd.blockiter import key_split
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    rng = random.Random(14)
    t = Table(table_bytes("cr_schema_000014.sst"))
    assert t.comparer() == C
    h0 = t.decode(resolve=False).to_host()
    keys = all_keys(h0)
    n = len(keys)
    bare = [k[:key_split(C, k)] for k in keys]
    mvcc = [k for k in keys if k and k[-1] in (9, 13)]
    assert mvcc

    def shift(k, dw):
        m = len(k) - k[-1]
        wall = int.from_bytes(k[m:m + 8], "big")
        return k[:m] + ((wall + dw) % (1 << 64)).to_bytes(8, "big") + k[m + 8:]

    pool = keys + bare + [shift(k, 1) for k in mvcc] + [shift(k, -1) for k in mvcc]
    lo = [rng.choice(pool) for _ in range(400)] + [None, keys[0], bare[n // 2]]
    up = [rng.choice(pool + [None]) for _ in range(400)] + [None, keys[-1], None]
    for resolve in (False, True):
        hh = t.decode(resolve=resolve).to_host()
        for hide in (False, True):
            r = device_result(t.scan(lo, up, hide_obsolete_points=hide, resolve=resolve))
            assert_same(r, scan_host(hh, lo, up, comparer=C, hide_obsolete_points=hide), ("crdb", resolve, hide))
        assert r[0]["status_mask"] == 0
    assert len(t._scan) == 2 and all(len(idx) == 2 for _, idx in t._scan.values())  # decoded and prepared once each
    r = device_result(t.scan(lo[:40], up[:40], resolve=False))
    assert_scan_is(r, expected_scan(h0, lo[:40], up[:40], C), C, "crdb walk")
    whole = device_result(t.scan([None], [None]))
    assert whole[0]["n_kv"] == n and whole[2].tolist() == list(range(n))


def test_mixed_batch_per_block():
    from pebble_amd.colblk import gen_col_blocks
    rb, ro, rl, _ = gen_row_blocks(1, 4, 8192, 16, 16, 100)
    cb, co, cl, _ = gen_col_blocks(1, 4, 8192)
    rows = [bytes(rb[ro[i]:ro[i] + rl[i]]) for i in range(4)]
    cols = [bytes(cb[co[i]:co[i] + cl[i]]) for i in range(4)]
    blocks = [x for p in zip(rows, cols) for x in p]
    fmts = [N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1] * 4
    d = dev_decode(blocks, N.PBL_FMT_ROW, block_format=fmts)
    h = d.to_host()
    assert h["status_mask"] == 0
    for comparer, sel in ((D, range(0, 8, 2)), (C, range(1, 8, 2))):
        lo, up, blk = [], [], []
        for b in sel:
            ks = block_keys(h, b)
            m = len(ks)
            lo += [None, ks[0], ks[m // 3], ks[-1], ks[m // 2][:-1]]
            up += [None, ks[-1], ks[2 * m // 3], None, ks[m // 2] + b"\x00"]
            blk += [b] * 5
        for hide in (False, True):
            check(d, h, lo, up, comparer, blocks=blk, hide=hide, ctx=("mixed", comparer))


# ---- 6. overflow ----------------------------------------------------------------------------
def test_overflow_writes_sizes_and_nothing_else():
    import torch
    from pebble_amd.batch import Capacity, DecodedBatch
    keys = [b"o%04d" % i for i in range(400)]
    d = dev_decode([row_block(keys[:150], 1), row_block(keys[150:], 151)])
    h = d.to_host()
    lo, up = [None, keys[100], keys[7]], [None, keys[390], keys[8]]
    full = scan_host(h, lo, up, comparer=D)[0]
    caps = (full["n_kv"], full["key_bytes_total"], full["val_bytes_total"])
    idx = prepare(d, D, False, 3)
    lb, lo_, ub, uo, fl = pack_bounds(lo, up)
    dev = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (lb, lo_, ub, uo, fl)]
    q = N.ScanQueriesC(*(x.data_ptr() for x in dev), None, 3, D, 0, 0)
    src = d.c_struct()
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        out = DecodedBatch.allocate(3, Capacity(cap[0], cap[1], cap[2], 0), "cuda", restarts=False)
        bufs = (out.trailer, out.kv_flags, out.entry_off, out.key_off, out.val_off, out.key_bytes, out.val_bytes)
        for x in bufs:
            x.view(torch.uint8).fill_(0xAA)
        skv = torch.full((caps[0],), -1, dtype=torch.int64, device="cuda")
        so = N.ScanOutC(out.c_struct(), None, skv.data_ptr())
        rc = N.lib().pbl_scan_batch(ctypes.byref(src), 2, idx.n_kv, ctypes.byref(q), ctypes.byref(so),
                                    ctypes.c_void_p(idx.workspace.data_ptr()), idx.workspace.numel(), 0, None)
        assert rc == N.PBL_OK
        torch.cuda.synchronize()
        t = out.read_totals()
        assert t.status_mask == 1 << N.PBL_OVERFLOW and (t.n_kv, t.key_bytes, t.val_bytes) == caps, short
        for k in ("blk_kv_base", "blk_key_base", "blk_val_base"):
            assert getattr(out, k).cpu().numpy().view(np.uint64).tolist() == full[k].tolist(), (short, k)
        assert out.blk_status.cpu().tolist() == [0, 0, 0]
        for x in bufs:
            assert bool((x.view(torch.uint8) == 0xAA).all()), short
        assert bool((skv == -1).all())
    # the same workspace, enough room: the result
    r = check(d, h, lo, up, D, index=idx, ctx="after overflow")
    assert r[0]["n_kv"] == caps[0]


# ---- 7. overlap -----------------------------------------------------------------------------
def test_overlapping_queries_each_get_a_copy():
    buf, off, lens, _ = gen_row_blocks(8, 4, 32768, 16, 16, 100, n_threads=4)
    d = dev_decode([bytes(buf[int(o): int(o) + int(n)]) for o, n in zip(off, lens)])
    h = d.to_host()
    n = h["n_kv"]
    keys = all_keys(h)
    lo = [None] * 64 + [keys[10], keys[10]]
    up = [None] * 64 + [keys[500], keys[500]]
    r = check(d, h, lo, up, D, ctx="overlap")
    assert r[0]["n_kv"] == 64 * n + 2 * 490 and r[0]["val_bytes_total"] >= 64 * h["val_bytes_total"]
    assert np.diff(r[0]["blk_kv_base"]).tolist() == [n] * 64 + [490, 490]
    assert result_kvs(r[0], 64) == result_kvs(r[0], 65)
    assert (r[2][:64 * n].reshape(64, n) == np.arange(n, dtype=np.uint64)).all()


# ---- 8. reuse and a stale index -------------------------------------------------------------
def test_reuse_and_stale_index():
    keys = [b"r%04d" % i for i in range(600)]
    obs = [i % 5 == 0 for i in range(600)]
    d = dev_decode([row_block(keys[:300], 1, obs[:300]), row_block(keys[300:], 301, obs[300:])])
    h = d.to_host()
    lo, up = [keys[3], None, keys[299]], [keys[580], keys[301], None]
    idx = prepare(d, D, True, 16)
    a = check(d, h, lo, up, D, hide=True, index=idx, ctx="first")
    b = check(d, h, lo[::-1], up[::-1], D, hide=True, index=idx, ctx="other queries")
    c = check(d, h, lo, up, D, hide=True, index=idx, ctx="second")
    assert_same(a, c, "reuse")
    assert result_kvs(b[0], 2) == result_kvs(a[0], 0)
    # a result is a decoded batch: scanned and sought again, per "block"
    res = scan(d, lo, up, comparer=D, hide_obsolete_points=True, index=idx)
    hr = res.batch.to_host()
    r2 = check(res.batch, hr, [keys[10], None], [keys[20], None], D, blocks=[0, 2], ctx="scan of a scan")
    assert [k for k, _, _, _ in result_kvs(r2[0], 0)] == [keys[i] for i in range(10, 20) if i % 5]
    assert result_kvs(r2[0], 1) == result_kvs(a[0], 2)
    # an index prepared for another comparer, or another hide flag: empty results, a status everywhere
    for stale in (dataclasses.replace(idx, comparer=T), ):
        r = device_result(scan(d, lo, up, comparer=T, hide_obsolete_points=True, index=stale))
        assert r[0]["blk_status"].tolist() == [N.PBL_INVALID_ARG] * 3 and r[0]["n_kv"] == 0
        assert r[0]["n_bad_blocks"] == 3 and r[0]["status_mask"] == 1 << N.PBL_INVALID_ARG
    stale = dataclasses.replace(idx, hide_obsolete_points=False)
    r = device_result(scan(d, lo, up, comparer=D, hide_obsolete_points=False, index=stale))
    assert r[0]["blk_status"].tolist() == [N.PBL_INVALID_ARG] * 3 and r[0]["n_kv"] == 0
