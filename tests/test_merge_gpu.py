"""Batched k-way merge on the device (pbl_merge_size / pbl_merge_batch,
pebble_amd/csrc/merge.hip) over batches decoded on the device.  The expected
result is the host's over to_host() of the same runs (pbl_merge_batch_host, a
different algorithm; every array compared exactly) and, on the hand-built cases
of mergeutil.cases(), also Python's `sorted` over pbl_key_compare."""
import ctypes

import numpy as np
import pytest

from mergeutil import BAD, C, D, S, assert_merge_is, assert_same, cases, device_result
from pebble_amd import _native as N
from pebble_amd.merge import merge, merge_host, merge_scan
from pebble_amd.rowblk import Writer, gen_row_blocks
from scanutil import ARRAYS, TOTALS, result_kvs

pytestmark = pytest.mark.gpu

CASES = cases()
POSITIONAL = N.PBL_KV_RESTART | N.PBL_KV_RESTART_SAMEPFX  # where a KV sits in its row block, not what it is


def dev_decode(blocks, fmt=N.PBL_FMT_ROW, block_format=None):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", fmt, 0, block_format=block_format))


def row_block(kvs, restart=4):
    w = Writer(restart)
    for k, t, v in kvs:
        w.add(k, t, v)
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def dev_run(blocks, restart=4):
    return dev_decode([corrupt(row_block([(b"x", S(1), b"")])) if b is None else row_block(b, restart) for b in blocks])


def check(runs, comparer, ctx="", python=False):
    """Device against pbl_merge_batch_host (every array) and, with `python`,
    against `sorted`; the source outputs name KVs whose bytes are the
    result's.  Returns (device result, the runs' host arrays)."""
    hosts = [d.to_host() for d in runs]
    r = device_result(merge(runs, comparer=comparer))
    assert_same(r, merge_host(hosts, comparer=comparer), ctx)
    if python:
        assert_merge_is(r, hosts, comparer, ctx)
    res, src_run, src_kv = r
    assert len(src_run) == len(src_kv) == res["n_kv"], ctx
    for q in range(len(res["blk_status"])):
        kv0 = int(res["blk_kv_base"][q])
        srcs = [result_kvs(h, q) if int(res["blk_status"][q]) == 0 else [] for h in hosts]
        for j, kv in enumerate(result_kvs(res, q)):
            run, at = int(src_run[kv0 + j]), int(src_kv[kv0 + j])
            assert kv == srcs[run][at - int(hosts[run]["blk_kv_base"][q])], (ctx, q, j, "src")
    return r, hosts


# ---- 1. the hand-built cases: device against host and against Python ----------------------------
@pytest.mark.parametrize("name,comparer,runs", CASES, ids=[c[0] for c in CASES])
def test_hand_built_cases(name, comparer, runs):
    devs = [dev_run(blocks, restart=(1, 4, 16)[r % 3]) for r, blocks in enumerate(runs)]
    r, hosts = check(devs, comparer, name, python=True)
    for h, blocks in zip(hosts, runs):  # the device decoded what the case says
        assert [int(s != 0) for s in h["blk_status"]] == [int(b is None) for b in blocks], name
        assert h["n_kv"] == sum(len(b) for b in blocks if b is not None), name
    st = r[0]["blk_status"].tolist()
    if name == "unsorted block":
        assert st == [0, N.PBL_INVALID_ARG, 0] and np.diff(r[0]["blk_kv_base"]).tolist() == [40, 0, 44]
    elif name == "unsorted trailers":
        assert st == [N.PBL_INVALID_ARG] and r[0]["n_kv"] == 0
    elif name == "bad block":
        assert st == [0, BAD, 0] and np.diff(r[0]["blk_kv_base"]).tolist() == [30, 0, 36]
    else:
        assert r[0]["status_mask"] == 0 and r[0]["n_kv"] == sum(h["n_kv"] for h in hosts), name


# ---- 2. colblk (crdb1) runs and a mixed pair ------------------------------------------------------
def _gen(seed, n=4):
    from pebble_amd.colblk import gen_col_blocks
    rb, ro, rl, _ = gen_row_blocks(seed, n, 8192, 16, 16, 100)
    cb, co, cl, _ = gen_col_blocks(seed, n, 8192)
    rows = [bytes(rb[int(ro[i]):int(ro[i]) + int(rl[i])]) for i in range(n)]
    cols = [bytes(cb[int(co[i]):int(co[i]) + int(cl[i])]) for i in range(n)]
    return rows, cols


def test_colblk_runs():
    """The generator's crdb1 blocks hold keys in bytewise order (they are not
    sorted under the crdb comparer, which both sides report alike); a real
    crdb table supplies runs that are."""
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    runs = [dev_decode(_gen(seed)[1], N.PBL_FMT_COL_CRDB1) for seed in (1, 2, 3)]
    r, hosts = check(runs, D, "crdb1 blocks")
    assert r[0]["status_mask"] == 0 and r[0]["n_kv"] == sum(h["n_kv"] for h in hosts) > 0
    assert set(r[1].tolist()) == {0, 1, 2}
    r, _ = check(runs, C, "crdb1 blocks, crdb comparer")
    assert set(r[0]["blk_status"].tolist()) <= {0, N.PBL_INVALID_ARG}
    t = Table(table_bytes("cr_schema_000014.sst"))
    assert t.comparer() == C
    d = t.decode(resolve=False)
    r, hosts = check([d, d, d], C, "crdb table", python=True)
    assert r[0]["status_mask"] == 0 and r[0]["n_kv"] == 3 * hosts[0]["n_kv"] > 0


def test_mixed_pair():
    runs = []
    for seed in (1, 2):
        rows, cols = _gen(seed)
        blocks = [x for p in zip(rows, cols) for x in p]
        runs.append(dev_decode(blocks, N.PBL_FMT_ROW, block_format=[N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1] * 4))
    r, hosts = check(runs, D, "mixed")
    assert r[0]["status_mask"] == 0 and r[0]["n_kv"] == sum(h["n_kv"] for h in hosts) > 0
    check(runs, C, "mixed, crdb comparer")


# ---- 3. the result reads as a decoded batch ---------------------------------------------------------
def _four_runs():
    _, comparer, runs = next(c for c in CASES if c[0] == "lengths K=16")
    return comparer, [dev_run(blocks) for blocks in runs[:4]]


def test_result_reads_as_a_decoded_batch():
    from pebble_amd.blockiter import DataIter
    from pebble_amd.scan import scan, scan_host
    from pebble_amd.seek import seek, seek_host
    comparer, runs = _four_runs()
    res = merge(runs, comparer=comparer)
    h = res.batch.to_host()
    nb = len(h["blk_status"])
    assert h["status_mask"] == 0
    keys, blocks = [], []
    for q in range(nb):
        kvs = result_kvs(h, q)
        it = DataIter(h, q, comparer)
        kv, j = it.First(), 0
        while kv is not None:
            assert (kv.user_key, kv.trailer, kv.value) == kvs[j][:3], (q, j)
            kv, j = it.Next(), j + 1
        assert j == len(kvs)
        for k in [x[0] for x in kvs[:: max(len(kvs) // 5, 1)]] + [b"", b"zzz"]:
            keys += [k, k + b"\x00"]
            blocks += [q, q]
    for op in ("ge", "lt"):
        got = seek(res.batch, keys, op=op, comparer=comparer, blocks=blocks)
        exp = seek_host(h, keys, op=op, comparer=comparer, blocks=blocks)
        assert got.kv.cpu().numpy().view(np.uint64).tolist() == exp[0].tolist(), op
        assert got.flags.cpu().numpy().tolist() == exp[2].tolist(), op
    lo, up = keys[0::2], keys[1::2][:-1] + [None]
    sr = scan(res.batch, lo, up, comparer=comparer, blocks=blocks[0::2])
    se = scan_host(h, lo, up, comparer=comparer, blocks=blocks[0::2])
    for k in ARRAYS:
        assert (np.asarray(sr.batch.to_host()[k]).astype(np.uint64) == np.asarray(se[0][k]).astype(np.uint64)).all(), k
    # merged again: alone it comes back as it is; with a run, the device and the host agree
    again = device_result(merge([res.batch], comparer=comparer))
    assert_same(again, (h, np.zeros(h["n_kv"], np.uint8), np.arange(h["n_kv"], dtype=np.uint64)), "alone")
    check([res.batch, runs[0]], comparer, "again")


def test_grouping():
    _, comparer, runs = next(c for c in CASES if c[0] == "equal internal keys")
    comparer2, four = _four_runs()
    tie = [dev_run(blocks) for blocks in runs] + [dev_run(runs[0])]
    for cmp_, (a, b, c, d) in ((comparer, tie), (comparer2, four)):
        flat = device_result(merge([a, b, c, d], comparer=cmp_))
        ab, cd = merge([a, b], comparer=cmp_).batch, merge([c, d], comparer=cmp_).batch
        nested = device_result(merge([ab, cd], comparer=cmp_))
        assert flat[0]["n_kv"] > 0 and flat[0]["status_mask"] == 0
        assert_same(nested, flat, "grouping", skip=("src",))


# ---- 4. end to end: decode -> scan -> merge ---------------------------------------------------------
def test_scans_of_dealt_tables_merge_to_the_scan_of_the_whole():
    """About 3,000 KVs in order, dealt round-robin into three tables' worth of
    row blocks; every array of the merged scans equals the scan of the undealt
    batch.  kv_flags is compared without PBL_KV_RESTART / RESTART_SAMEPFX: those
    two bits say where a KV sits in its row block (the three tables use restart
    intervals 1, 4 and 16), so they differ between the two encodings by
    construction; that they travel unchanged is checked through src_run /
    src_kv."""
    from pebble_amd.scan import scan
    n = 3001
    kvs = [(b"e%05d" % (i // 2), S(2 * n - i), b"val%d" % i * (1 + i % 5)) for i in range(n)]
    whole = dev_decode([row_block(kvs[i:i + 300], 8) for i in range(0, n, 300)])
    tables = []
    for r, restart in enumerate((1, 4, 16)):
        mine = kvs[r::3]
        size = (130, 256, 77)[r]
        tables.append(dev_decode([row_block(mine[i:i + size], restart) for i in range(0, len(mine), size)]))
    edges = [0, 1, 63, 64, 255, 256, 257, 299, 300, 301, 511, 512, 513, 768, 1000, 2999, 3000]
    lo, up = [None], [None]
    for i, a in enumerate(edges):
        for b in (edges[(i + 1) % len(edges)], edges[(i + 5) % len(edges)]):
            lo.append(kvs[a][0])
            up.append(kvs[b][0] if b > a else None)
    lo += [kvs[700][0], b"zz"]
    up += [kvs[700][0], None]  # empty ranges
    assert 36 <= len(lo) <= 44
    exp = scan(whole, lo, up, comparer=D).batch.to_host()
    scans = [scan(t, lo, up, comparer=D) for t in tables]
    res = merge([s.batch for s in scans], comparer=D)
    got, src_run, src_kv = device_result(res)
    assert got["status_mask"] == 0 and got["n_kv"] == exp["n_kv"] > n
    for k in ARRAYS:
        x, y = np.asarray(got[k]).astype(np.uint64), np.asarray(exp[k]).astype(np.uint64)
        if k == "kv_flags":
            x, y = x & ~np.uint64(POSITIONAL), y & ~np.uint64(POSITIONAL)
        assert x.shape == y.shape and (x == y).all(), k
    for k in TOTALS:
        assert int(got[k]) == int(exp[k]), k
    hs = [s.batch.to_host() for s in scans]
    for r in range(3):
        m = src_run == r
        assert (got["kv_flags"][m] == hs[r]["kv_flags"][src_kv[m].astype(np.int64)]).all(), r
        assert (got["entry_off"][m] == hs[r]["entry_off"][src_kv[m].astype(np.int64)]).all(), r
    assert (src_run[: exp["n_kv"]][:n] == np.arange(n) % 3).all()  # the first range is the whole table


def test_merge_scan_on_real_tables():
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    data = table_bytes("h_no_compression.sst")
    t0, t1 = Table(data), Table(data)
    one = t0.scan([None], [None]).batch.to_host()
    n = one["n_kv"]
    assert n > 0
    got, src_run, src_kv = device_result(merge_scan([t0, t1], [None], [None]))
    assert got["n_kv"] == 2 * n and got["status_mask"] == 0
    kvs = result_kvs(one, 0)
    assert result_kvs(got, 0) == [kv for kv in kvs for _ in (0, 1)]
    assert src_run.tolist() == [0, 1] * n and src_kv.tolist() == [i for i in range(n) for _ in (0, 1)]

    class Other(Table):
        def comparer(self):
            return (super().comparer() + 1) % 3

    with pytest.raises(ValueError):
        merge_scan([t0, Other(data)], [None], [None])


# ---- 5. overflow -------------------------------------------------------------------------------------
def test_overflow_writes_sizes_and_nothing_else():
    import torch
    from pebble_amd.batch import Capacity, DecodedBatch
    _, comparer, case = next(c for c in CASES if c[0] == "lengths K=3")
    runs = [dev_run(blocks) for blocks in case]
    hosts = [d.to_host() for d in runs]
    full = merge_host(hosts, comparer=comparer)[0]
    caps = (full["n_kv"], full["key_bytes_total"], full["val_bytes_total"])
    nb, n_kv = runs[0].n_blocks, sum(h["n_kv"] for h in hosts)
    structs = (N.DecodeOutC * 3)(*[d.c_struct() for d in runs])
    rs = N.MergeRunsC(ctypes.cast(structs, ctypes.POINTER(N.DecodeOutC)), 3, nb, comparer, 0, n_kv)
    ws = torch.empty(int(N.lib().pbl_merge_workspace_bytes(3, nb, n_kv)), dtype=torch.uint8, device="cuda")
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        out = DecodedBatch.allocate(nb, Capacity(cap[0], cap[1], cap[2], 0), "cuda", restarts=False)
        bufs = (out.trailer, out.kv_flags, out.entry_off, out.key_off, out.val_off, out.key_bytes, out.val_bytes)
        for x in bufs:
            x.view(torch.uint8).fill_(0xAA)
        sr = torch.full((caps[0],), 0xAA, dtype=torch.uint8, device="cuda")
        sk = torch.full((caps[0],), -1, dtype=torch.int64, device="cuda")
        mo = N.MergeOutC(out.c_struct(), sr.data_ptr(), sk.data_ptr())
        rc = N.lib().pbl_merge_batch(ctypes.byref(rs), ctypes.byref(mo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0,
                                     None)
        assert rc == N.PBL_OK
        torch.cuda.synchronize()
        t = out.read_totals()
        assert t.status_mask == 1 << N.PBL_OVERFLOW and (t.n_kv, t.key_bytes, t.val_bytes) == caps, short
        for k in ("blk_kv_base", "blk_key_base", "blk_val_base"):
            assert getattr(out, k).cpu().numpy().view(np.uint64).tolist() == full[k].tolist(), (short, k)
        assert out.blk_status.cpu().tolist() == [0] * nb
        for x in bufs:
            assert bool((x.view(torch.uint8) == 0xAA).all()), short
        assert bool((sr == 0xAA).all()) and bool((sk == -1).all())
    # the same workspace, enough room, in one call (no size pass before it)
    out = DecodedBatch.allocate(nb, Capacity(caps[0], caps[1], caps[2], 0), "cuda", restarts=False)
    mo = N.MergeOutC(out.c_struct(), None, None)
    assert N.lib().pbl_merge_batch(ctypes.byref(rs), ctypes.byref(mo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0,
                                   None) == N.PBL_OK
    torch.cuda.synchronize()
    got = out.to_host()
    for k in ARRAYS:
        assert (np.asarray(got[k]).astype(np.uint64) == np.asarray(full[k]).astype(np.uint64)).all(), k
