"""Batched SeekGE / SeekLT on the device (pbl_seek_prepare / pbl_seek_batch,
pebble_amd/csrc/seek.hip) over batches decoded on the device.  The expected
result is always the host's over to_host() of the same decoded batch:
pbl_seek_batch_host for whole query sets and, for the hand-built cases, the
one-key iterator DataIter (tests/seekutil.expected); kv, block and flags are
compared exactly."""
import random
import struct

import numpy as np
import pytest

from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, gen_row_blocks, make_trailer
from pebble_amd.seek import prepare, seek, seek_host
from seekutil import assert_seek, block_keys, device_result, expected, trailer_index

pytestmark = pytest.mark.gpu

D, T, C = N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB


def dev_decode(blocks, fmt=N.PBL_FMT_ROW, block_format=None, flags=0):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", fmt, flags, block_format=block_format))


def row_block(keys, seq0, obsolete=None, restart=4):
    w = Writer(restart)
    for i, k in enumerate(keys):
        w.add_with_optional_value_prefix(k, make_trailer(seq0 + i, 1), bool(obsolete and obsolete[i]), b"v%d" % i,
                                         len(k), False, 0, False)
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def both(d, h, keys, comparer, blocks=None, hide=False, index=None, ctx=""):
    """Device against pbl_seek_batch_host, both ops; returns the device results."""
    out = {}
    for op in ("ge", "lt"):
        r = device_result(seek(d, keys, op=op, comparer=comparer, blocks=blocks, hide_obsolete_points=hide,
                               index=index))
        e = seek_host(h, keys, op=op, comparer=comparer, blocks=blocks, hide_obsolete_points=hide)
        assert_seek(r, [x.tolist() for x in e], (ctx, op, hide))
        out[op] = r
    return out


# ---- 1. chunk boundaries, default comparer, per-block mode ---------------------------
def test_chunk_boundaries_per_block():
    pfx = b"0123456789abcdefghijklmnopqrstuvwxyz_"  # 37 bytes: every compare loops past two 16-B chunks
    assert len(pfx) == 37
    long_keys = [pfx + struct.pack(">I", 7 * i)[1:] for i in range(40)]
    a_keys = [b"a" * k for k in range(1, 35)]  # prefixes of each other across 15/16/17 and 31/32/33
    blocks = [row_block(long_keys, 1), row_block(a_keys, 1000), row_block([b"m"], 2000),
              corrupt(row_block([b"x", b"y"], 3000))]
    d = dev_decode(blocks)
    h = d.to_host()
    assert h["blk_status"].tolist()[:3] == [0, 0, 0] and int(h["blk_status"][3]) != 0
    base = long_keys + a_keys + [b"m"]
    probes = base + [k + b"\x00" for k in base] + [k[:-1] for k in base] + [b"", b"\xff" * 40]
    keys, blk = [], []
    for b in range(len(blocks) + 1):  # block 4 is past n_blocks
        keys += probes
        blk += [b] * len(probes)
    tidx = trailer_index(h)
    for n in (1, 63, 65, len(keys)):  # partial waves
        for op in ("ge", "lt"):
            r = device_result(seek(d, keys[:n], op=op, comparer=D, blocks=blk[:n]))
            assert_seek(r, expected(h, keys[:n], op, D, blk[:n], False, tidx), (n, op))
    # a slice that starts in the middle, so that the short launches see every block too
    for lo in (len(probes) - 30, 3 * len(probes) - 5):
        r = device_result(seek(d, keys[lo:lo + 65], op="ge", comparer=D, blocks=blk[lo:lo + 65]))
        assert_seek(r, expected(h, keys[lo:lo + 65], "ge", D, blk[lo:lo + 65], False, tidx), lo)
    r = device_result(seek(d, probes, op="ge", comparer=D, blocks=[3] * len(probes)))
    assert (r[0] == np.uint64(N.PBL_SEEK_NONE)).all() and (r[2] == N.PBL_SEEK_BAD_BLOCK).all()
    r = device_result(seek(d, probes, op="lt", comparer=D, blocks=[4] * len(probes)))
    assert (r[0] == np.uint64(N.PBL_SEEK_NONE)).all() and (r[2] == N.PBL_SEEK_BAD_BLOCK).all()


# ---- 2. table mode over generated row blocks ------------------------------------------
@pytest.fixture(scope="module")
def gen64():
    buf, off, lens, _ = gen_row_blocks(8, 64, 32768, 16, 16, 100, n_threads=4)
    return [bytes(buf[int(o): int(o) + int(n)]) for o, n in zip(off, lens)]


def _table_queries(h, rng):
    nb = len(h["blk_status"])
    firsts, lasts = [], []
    for b in range(nb):
        if int(h["blk_status"][b]) == 0:
            ks = block_keys(h, b)
            firsts.append(ks[0])
            lasts.append(ks[-1])
    allk = [k for b in range(nb) if int(h["blk_status"][b]) == 0 for k in block_keys(h, b)]
    edge = firsts + lasts + [k + b"\x00" for k in lasts] + [bytes(16), b"\xff" * 17]
    rnd = []
    for _ in range(1000):
        k = rng.choice(allk)
        rnd.append(k)
        rnd.append(rng.choice([k[:-1], k + b"\x01", k[:8], k[:15] + bytes([k[15] ^ 1])]))
    return firsts, lasts, edge, rnd


def test_table_mode_generated_rows(gen64):
    rng = random.Random(21)
    d = dev_decode(gen64)
    h = d.to_host()
    assert h["status_mask"] == 0
    firsts, lasts, edge, rnd = _table_queries(h, rng)
    idx = prepare(d, D)
    r = both(d, h, edge + rnd, D, index=idx, ctx="gen64")
    # the edges again from the one-key iterator
    tidx = trailer_index(h)
    for op in ("ge", "lt"):
        got = tuple(x[:len(edge)] for x in r[op])
        assert_seek(got, expected(h, edge, op, D, None, False, tidx), ("edge", op))
    nb, nf = 64, len(firsts)
    base = h["blk_kv_base"].astype(np.int64)
    ge, lt = r["ge"], r["lt"]
    # last key + "\0" lands on the next block's first KV; the first key under LT on the previous block's last
    for b in range(nb - 1):
        assert int(ge[0][2 * nf + b]) == base[b + 1] and int(ge[1][2 * nf + b]) == b + 1
        assert int(lt[0][b + 1]) == base[b + 1] - 1 and int(lt[1][b + 1]) == b
    assert int(ge[0][2 * nf + nb - 1]) == N.PBL_SEEK_NONE           # past the last key of the batch
    assert int(lt[0][3 * nf]) == N.PBL_SEEK_NONE and int(ge[0][3 * nf]) == 0     # below everything
    assert int(ge[0][3 * nf + 1]) == N.PBL_SEEK_NONE and int(lt[0][3 * nf + 1]) == base[nb] - 1  # above everything
    assert (ge[2][:2 * nf] == (N.PBL_SEEK_EXACT | N.PBL_SEEK_SAME_PREFIX)).all()
    # a second seek on the same prepare: identical
    r2 = both(d, h, edge + rnd, D, index=idx, ctx="again")
    for op in ("ge", "lt"):
        for x, y in zip(r[op], r2[op]):
            assert (x == y).all()


def test_table_mode_passes_over_a_corrupt_block(gen64):
    rng = random.Random(22)
    blocks = gen64[:32] + [corrupt(gen64[5])] + gen64[32:]
    d = dev_decode(blocks)
    h = d.to_host()
    assert int(h["blk_status"][32]) != 0 and h["n_bad_blocks"] == 1
    assert int(h["blk_kv_base"][33]) == int(h["blk_kv_base"][32])  # a corrupt block owns no KV index
    firsts, lasts, edge, rnd = _table_queries(h, rng)
    r = both(d, h, edge + rnd[:600], D, ctx="corrupt")
    tidx = trailer_index(h)
    q = [lasts[31] + b"\x00", firsts[32]]  # across the corrupt block, both ways
    ge = device_result(seek(d, q, op="ge", comparer=D))
    lt = device_result(seek(d, q, op="lt", comparer=D))
    assert_seek(ge, expected(h, q, "ge", D, None, False, tidx))
    assert_seek(lt, expected(h, q, "lt", D, None, False, tidx))
    assert int(ge[1][0]) == 33 and int(lt[1][1]) == 31
    assert not (r["ge"][1] == 32).any() and not (r["lt"][1] == 32).any()


# ---- 3. HideObsoletePoints across block boundaries ---------------------------------------
def test_hidden_runs_cross_blocks():
    b0, b1, b2 = [b"a1", b"a2", b"a3", b"a4"], [b"b1", b"b2", b"b3"], [b"c1", b"c2", b"c3"]
    blocks = [row_block(b0, 1, [0, 0, 1, 1]), row_block(b1, 100, [1, 1, 1]), row_block(b2, 200, [1, 0, 0])]
    d = dev_decode(blocks)
    h = d.to_host()
    tidx = trailer_index(h)
    probes = b0 + b1 + b2 + [b"", b"a", b"b", b"c", b"d"]
    for hide in (False, True):
        for op in ("ge", "lt"):
            r = device_result(seek(d, probes, op=op, comparer=D, hide_obsolete_points=hide))
            assert_seek(r, expected(h, probes, op, D, None, hide, tidx), ("table", op, hide))
            for b in range(3):
                r = device_result(seek(d, probes, op=op, comparer=D, blocks=[b] * len(probes),
                                       hide_obsolete_points=hide))
                assert_seek(r, expected(h, probes, op, D, [b] * len(probes), hide, tidx), (b, op, hide))
    r = device_result(seek(d, [b"a4"], op="ge", comparer=D, hide_obsolete_points=True))
    assert (int(r[0][0]), int(r[1][0])) == (8, 2)   # c2, in block 2
    r = device_result(seek(d, [b"c2"], op="lt", comparer=D, hide_obsolete_points=True))
    assert (int(r[0][0]), int(r[1][0])) == (1, 0)   # a2, in block 0
    r = device_result(seek(d, [b"a4"], op="ge", comparer=D, blocks=[0], hide_obsolete_points=True))
    assert int(r[0][0]) == N.PBL_SEEK_NONE and int(r[2][0]) == 0
    r = device_result(seek(d, [b"c2"], op="lt", comparer=D, blocks=[2], hide_obsolete_points=True))
    assert int(r[0][0]) == N.PBL_SEEK_NONE and int(r[2][0]) == 0


def test_hidden_generated_rows():
    rng = random.Random(31)
    buf, off, lens, _ = gen_row_blocks(9, 16, 32768, 16, 16, 100, n_threads=4, obsolete_every=3)
    d = dev_decode([bytes(buf[int(o): int(o) + int(n)]) for o, n in zip(off, lens)])
    h = d.to_host()
    assert (h["kv_flags"] & N.PBL_KV_OBSOLETE).any()
    _, _, edge, rnd = _table_queries(h, rng)
    q = edge + rnd[:1000]
    both(d, h, q, D, hide=True, ctx="obs table")
    blk = [rng.randrange(16) for _ in q]
    both(d, h, q, D, blocks=blk, hide=True, ctx="obs block")
    tidx = trailer_index(h)
    for op in ("ge", "lt"):
        r = device_result(seek(d, edge, op=op, comparer=D, hide_obsolete_points=True))
        assert_seek(r, expected(h, edge, op, D, None, True, tidx), ("obs edge", op))


# ---- 4. testkeys comparer over colblk DefaultKeySchema blocks ---------------------------
def test_testkeys_suffix_order():
    from pebble_amd.colblk import SCHEMA_DEFAULT, DataBlockEncoder
    P = b"c_prefix_longer_than_sixteen_bytes_"  # (sorts after block 0's keys: the batch is ordered)
    b0 = [b"a", b"a@10", b"a@3", b"b@5", b"b@5_synthetic"]
    b1 = [P + b"a@9", P + b"a@2", P + b"b", P + b"b@100", P + b"b@20"]
    blocks, seq = [], 1
    for ks in (b0, b1):
        w = DataBlockEncoder(SCHEMA_DEFAULT, 16)
        for k in ks:
            w.add(k, make_trailer(seq, 1), b"v")
            seq += 1
        blocks.append(w.finish())
    d = dev_decode(blocks, N.PBL_FMT_COL_DEFAULT)
    h = d.to_host()
    assert h["status_mask"] == 0 and block_keys(h, 0) == b0 and block_keys(h, 1) == b1
    tidx = trailer_index(h)
    probes = [b"a@7", b"a@100", b"a@3", b"a", b"b", b"b@4", b"b@5", b"c", b"",
              P + b"a@5", P + b"a@9", P + b"a", P + b"b@50", P + b"b@1", P + b"c", P[:-1], P[:16], P[:17]]
    for op in ("ge", "lt"):
        r = device_result(seek(d, probes, op=op, comparer=T))
        assert_seek(r, expected(h, probes, op, T, None, False, tidx), ("tk table", op))
        for b in (0, 1):
            r = device_result(seek(d, probes, op=op, comparer=T, blocks=[b] * len(probes)))
            assert_seek(r, expected(h, probes, op, T, [b] * len(probes), False, tidx), ("tk block", b, op))
    r = device_result(seek(d, [b"a@7", b"a@100", b"a@3"], op="ge", comparer=T))
    # "@10" sorts before "@3": a bytewise shortcut would land a@7 past a@3
    assert r[0].tolist() == [2, 1, 2] and r[2].tolist()[2] == N.PBL_SEEK_EXACT | N.PBL_SEEK_SAME_PREFIX


# ---- 5. crdb comparer, the reference table ------------------------------------------------
def test_crdb_reference_table():
    import torch
    from pebble_amd.blockiter import key_split
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    t = Table(table_bytes("cr_schema_000014.sst"))
    assert t.comparer() == C
    h = t.decode(resolve=False).to_host()
    nb = len(h["blk_status"])
    keys = [k for b in range(nb) for k in block_keys(h, b)]
    assert len(keys) == h["n_kv"] > 0
    bare = [k[:key_split(C, k)] for k in keys]
    mvcc = [k for k in keys if k and k[-1] in (9, 13)]
    assert mvcc

    def shift(k, dw):
        n = len(k) - k[-1]
        wall = int.from_bytes(k[n:n + 8], "big")
        return k[:n] + ((wall + dw) % (1 << 64)).to_bytes(8, "big") + k[n + 8:]

    shifted = [shift(k, 1) for k in mvcc] + [shift(k, -1) for k in mvcc]
    wall8 = [k for k in keys if k and k[-1] == 9]
    zero_logical = [k[:-1] + bytes(4) + b"\x0d" for k in wall8]
    probes = keys + bare + shifted + zero_logical
    for op, fn in (("ge", t.seek_ge), ("lt", t.seek_lt)):
        r = device_result(fn(probes))
        e = seek_host(h, probes, op=op, comparer=C)
        assert_seek(r, [x.tolist() for x in e], ("crdb", op))
    tidx = trailer_index(h)
    sample = probes[:: max(1, len(probes) // 300)]
    assert_seek(device_result(t.seek_ge(sample)), expected(h, sample, "ge", C, None, False, tidx), "crdb iter ge")
    assert_seek(device_result(t.seek_lt(sample)), expected(h, sample, "lt", C, None, False, tidx), "crdb iter lt")
    # normalizeEngineSuffixForCompare: the 12-byte zero-logical form of an 8-byte version is the same key
    if zero_logical:
        r = device_result(t.seek_ge(zero_logical))
        assert (r[2] & N.PBL_SEEK_EXACT).all()
    g = t.get(keys).cpu().numpy()
    from pebble_amd.blockiter import key_compare
    own = np.arange(len(keys))
    first_of_run = np.array([i == 0 or key_compare(C, keys[i - 1], keys[i]) != 0 for i in range(len(keys))])
    assert (g[first_of_run] == own[first_of_run]).all() and (g >= 0).all()
    e_kv, _, e_fl = seek_host(h, shifted, op="ge", comparer=C)
    absent = (e_fl & N.PBL_SEEK_EXACT) == 0
    gs = t.get(shifted).cpu().numpy()
    assert absent.any() and (gs[absent] == -1).all() and (gs[~absent] == e_kv[~absent].astype(np.int64)).all()
    assert isinstance(t.get(keys), torch.Tensor)
    # a batch whose values were resolved seeks too (per-block mode)
    d2 = t.decode(resolve=True)
    h2 = d2.to_host()
    blk = [b for b in range(nb) for _ in block_keys(h, b)]
    both(d2, h2, keys, C, blocks=blk, ctx="resolved")


def test_unknown_comparer_is_an_error():
    from pebble_amd.batch import DecodeError
    from pebble_amd.sstable import COMPARER_PROP, Table
    from tableutil import table_bytes
    t = Table(table_bytes("cr_schema_000014.sst"))
    t._props = dict(t.properties())
    t._props[COMPARER_PROP] = b"some.other.comparer"
    with pytest.raises(DecodeError):
        t.seek_ge([b"k"])


# ---- 6. mixed row + colblk batch -------------------------------------------------------------
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
        keys, blk = [], []
        for b in sel:
            ks = block_keys(h, b)
            keys += ks + [ks[0][:-1], ks[-1] + b"\x00"]
            blk += [b] * (len(ks) + 2)
        both(d, h, keys, comparer, blocks=blk, ctx=("mixed", comparer))
        both(d, h, keys, comparer, blocks=blk, hide=True, ctx=("mixed hide", comparer))
