"""Pebblev8 tiering metadata on the device (PBL_COL_TIERING): every decode path
writes each colblk KV's KVMeta (DataBlockIter.NextWithMeta, sstable/colblk/
data_block.go:1574-1641) into tiering_span_id / tiering_attr, bit-exact against
the oracle, on the reference's own v8 blocks (writer_tiering_histogram), on
random v8 blocks (parity unpinned beyond the restatement: the reference holds
no other tiering bytes), on mixed batches (row KVs: KVMeta{}), under
HideObsoletePoints, through the device transforms and the blockiter adapter,
and on a full-size config-3-shaped batch with tiering columns."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import oracle
from colutil import build_block, build_block_meta, random_metas, random_rows
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, decode
from pebble_amd.colblk import SCHEMA_CRDB1, SCHEMA_DEFAULT, gen_col_blocks
from pebble_amd.rowblk import gen_row_blocks
from test_rowblk_gpu import ARRAYS, assert_same, pack

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "colblk_golden.json")
T = N.PBL_COL_TIERING
META = ("tiering_span_id", "tiering_attr")


def gpu(buf, off, lens, fmt, flags, block_fmt=None, meta=True, exact=False):
    b = BlockBatch.from_host(buf, off, lens, "cuda", fmt, flags, block_format=block_fmt)
    return decode(b, meta=meta, exact=exact).to_host()


def check(buf, off, lens, fmt, flags, block_fmt=None, ctx="", exact=False):
    o = oracle.decode_batch(buf, off, lens, fmt, block_fmt, flags, meta=True)
    g = gpu(buf, off, lens, fmt, flags, block_fmt, exact=exact)
    assert_same(g, o, ctx)
    for k in META:
        assert np.array_equal(g[k], o[k]), (ctx, k)
    return g


def test_reference_v8_blocks():
    with open(GOLDEN) as f:
        cases = json.load(f)["tiering"]["blocks"]
    blocks = [bytes.fromhex(c["block"]) for c in cases]
    for flags in (T, 0, T | N.PBL_KERNEL_SINGLE, T | N.PBL_KERNEL_PIPE, T | N.PBL_ROW_HIDE_OBSOLETE):
        g = check(*pack(blocks), SCHEMA_DEFAULT, flags, ctx=f"golden v8 flags={flags:#x}")
        want = [(r["span"], r["attr"]) if flags & T else (0, 0) for c in cases for r in c["rows"]]
        assert list(zip(g["tiering_span_id"].tolist(), g["tiering_attr"].tolist())) == want


@pytest.mark.parametrize("schema", [SCHEMA_DEFAULT, SCHEMA_CRDB1])
def test_random_v8_blocks(schema):
    rng = random.Random(600 + schema)
    blocks = []
    for _ in range(150):
        n = rng.choice([1, 2, 17, 100, 255, 256, 257, 700])
        rows = random_rows(rng, schema, n, shared=rng.choice([0, 3]), val_len=(0, rng.choice([1, 40, 300])))
        blk, _, _ = build_block_meta(schema, rows, random_metas(rng, len(rows)), rng.choice([1, 16, 64]))
        blocks.append(blk)
    buf, off, lens = pack(blocks)
    for flags in (T, T | N.PBL_KERNEL_SINGLE, T | N.PBL_KERNEL_PIPE, T | N.PBL_ROW_HIDE_OBSOLETE, T | N.PBL_BATCH_VARLEN):
        check(buf, off, lens, schema, flags, ctx=f"random v8 schema={schema} flags={flags:#x}")


def test_meta_arrays_without_tiering_and_v7_blocks():
    rng = random.Random(5)
    v7 = [build_block(SCHEMA_CRDB1, random_rows(rng, SCHEMA_CRDB1, rng.randint(1, 300)))[0] for _ in range(40)]
    buf, off, lens = pack(v7)
    g = check(buf, off, lens, SCHEMA_CRDB1, 0, ctx="v7 no tiering")
    assert g["n_kv"] > 0 and not g["tiering_span_id"].any() and not g["tiering_attr"].any()
    # the tiering config on blocks without the columns: initTieringMetadata's panic
    g = check(buf, off, lens, SCHEMA_CRDB1, T, ctx="v7 with tiering")
    assert g["status_mask"] == 1 << N.PBL_CORRUPT_COLBLK_HEADER and g["n_kv"] == 0


def test_corrupt_tiering_columns():
    rng = random.Random(8)
    blocks = []
    for i in range(60):
        rows = random_rows(rng, SCHEMA_DEFAULT, rng.randint(1, 200))
        blk = bytearray(build_block_meta(SCHEMA_DEFAULT, rows, random_metas(rng, len(rows)))[0])
        for _ in range(rng.randint(0, 3)):  # damage the end of the block (the tiering columns)
            blk[len(blk) - 1 - rng.randrange(min(64, len(blk)))] = rng.randrange(256)
        if i % 5 == 0:
            h = 4 + 7 + 5 * (2 + 5 + rng.randrange(2))
            blk[h] = rng.choice([1, 3])  # a tiering column of the wrong type
        blocks.append(bytes(blk))
    buf, off, lens = pack(blocks)
    for flags in (T, T | N.PBL_KERNEL_SINGLE, T | N.PBL_KERNEL_PIPE, T | N.PBL_ROW_HIDE_OBSOLETE):
        g = check(buf, off, lens, SCHEMA_DEFAULT, flags, ctx=f"corrupt v8 flags={flags:#x}")
        assert g["status_mask"] & (1 << N.PBL_CORRUPT_COLBLK_HEADER)


@pytest.mark.parametrize("flags", [T, T | N.PBL_ROW_HIDE_OBSOLETE])
def test_mixed_batches(flags):
    rng = random.Random(flags)
    rb, ro, rl, _ = gen_row_blocks(9, 64, 8192, 16, 16, 100)
    blocks, fmts = [], []
    for i in range(160):
        if i % 3 == 0:
            j = rng.randrange(64)
            blocks.append(rb[int(ro[j]):int(ro[j]) + int(rl[j])].tobytes())
            fmts.append(N.PBL_FMT_ROW)
        else:
            schema = rng.choice([SCHEMA_DEFAULT, SCHEMA_CRDB1])
            rows = random_rows(rng, schema, rng.randint(1, 300))
            blocks.append(build_block_meta(schema, rows, random_metas(rng, len(rows)))[0])
            fmts.append(schema)
    buf, off, lens = pack(blocks)
    g = check(buf, off, lens, N.PBL_FMT_ROW, flags, np.array(fmts, np.uint8), ctx=f"mixed v8 {flags:#x}")
    kvb = g["blk_kv_base"]
    for b, f in enumerate(fmts):
        if f == N.PBL_FMT_ROW:
            assert not g["tiering_attr"][kvb[b]:kvb[b + 1]].any()


def test_row_batch_meta_is_zero():
    buf, off, lens, n = gen_row_blocks(3, 512, 32768, 16, 16, 100)
    g = check(buf, off, lens, N.PBL_FMT_ROW, T, ctx="row batch with meta")
    assert g["n_kv"] == n and not g["tiering_span_id"].any() and not g["tiering_attr"].any()


def test_transforms_carry_meta():
    from pebble_amd.transforms import Transforms, apply_transforms
    rng = random.Random(12)
    blocks = []
    for _ in range(50):
        rows = random_rows(rng, SCHEMA_CRDB1, rng.randint(1, 250))
        blocks.append(build_block_meta(SCHEMA_CRDB1, rows, random_metas(rng, len(rows)))[0])
    buf, off, lens = pack(blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", SCHEMA_CRDB1, T), meta=True)
    h = d.to_host()
    t = apply_transforms(d, Transforms(synthetic_seq_num=7, hide_obsolete_points=True)).to_host()
    keep = (h["kv_flags"] & N.PBL_KV_OBSOLETE) == 0
    assert t["n_kv"] == int(keep.sum())
    assert np.array_equal(t["tiering_span_id"], h["tiering_span_id"][keep])
    assert np.array_equal(t["tiering_attr"], h["tiering_attr"][keep])


def test_blockiter_with_meta():
    """TestDataBlockIterWithMeta (data_block_meta_test.go:19-70) through the
    device decode and the blockiter adapter's *WithMeta calls."""
    from pebble_amd.blockiter import DataIter
    from pebble_amd.colblk import DataBlockEncoder
    w = DataBlockEncoder(SCHEMA_DEFAULT, 16, tiering=True)
    metas = [(42, 100), (43, 200), (0, 0)]
    for i, (k, m) in enumerate(zip((b"a", b"b", b"c"), metas)):
        w.add(k, (i + 1) << 8 | 1, b"value", meta=m)
    d = decode(BlockBatch.from_blocks([w.finish()], fmt=SCHEMA_DEFAULT, flags=T), meta=True).to_host()
    it = DataIter(d, 0, N.PBL_CMP_TESTKEYS)
    got = [it.FirstWithMeta()] + [it.NextWithMeta() for _ in range(2)]
    assert [m for _, m in got] == metas and all(kv is not None for kv, _ in got)
    assert it.NextWithMeta() == (None, (0, 0))
    kv, m = it.SeekGEWithMeta(b"b")
    assert kv.user_key == b"b" and m == (43, 200)
    assert it.SeekGEWithMeta(b"z") == (None, (0, 0))


def test_size_pass_with_tiering():
    buf, off, lens, n = gen_col_blocks(21, 256, tiering=4)
    g = check(buf, off, lens, SCHEMA_CRDB1, T, ctx="exact", exact=True)
    assert g["n_kv"] == n


@pytest.mark.timeout(600)
def test_config3_tiering_full_size():
    """BASELINE config 3's shape (64 Ki x 32 KiB crdb1 blocks) written as
    Pebblev8 blocks with tiering columns: every array, the meta included, equal
    to the oracle by SHA-256."""
    buf, off, lens, n = gen_col_blocks(33, 65536, tiering=4, n_threads=16)
    o = oracle.decode_batch(buf, off, lens, SCHEMA_CRDB1, None, T, meta=True)
    g = gpu(buf, off, lens, SCHEMA_CRDB1, T)
    assert g["n_kv"] == n == o["n_kv"] and g["status_mask"] == 0
    for k in ARRAYS + list(META):
        if g.get(k) is not None:
            assert hashlib.sha256(g[k].tobytes()).digest() == hashlib.sha256(o[k].tobytes()).digest(), k
    assert np.count_nonzero(g["tiering_attr"]) > 0.85 * n
