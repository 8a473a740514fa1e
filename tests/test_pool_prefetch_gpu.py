"""The staging-pool row kernel (rowblk_pool.hip.h) where a wave decodes more
than one block: the early release of the stage after the walk (PBL_POOL_EARLYREL)
and, in builds with PBL_POOL_PREFETCH, the next block staged under the emit's
last step.  The chip runs 2,048 pool waves, so a
wave reaches its second block (and the hand-over of a prefetched stage) only
in batches well past 2,048 blocks: about 8 Ki blocks of 2-4 KiB each, against
the oracle, bit-exact on every output array.

The block kinds that leave the fast path or the early release (a run longer
than the 16 parked entries, more entries than a slot holds, 3-byte header
varints, a block past the 32 KiB stage, an empty block, a corrupt restart
table, shared > len(previous key)) are interleaved every few blocks, so each
shows up both as the block a wave is emitting and as the one it staged ahead."""
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, gen_row_blocks, make_trailer
from rowutil import header_cases, mvcc_block
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
POOL = N.PBL_KERNEL_POOL
NB = 8192 + 3  # the last tickets are drawn by waves that already hold a prefetched stage or find none


def blocks_of(buf, off, lens):
    return [bytes(buf[int(o):int(o) + int(n)]) for o, n in zip(off, lens)]


def uniform(seed, n, size=4096, kl=16, vl=100):
    """Config-2-shaped blocks (restart interval 16), small."""
    return gen_row_blocks(seed, n, size, 16, kl, vl)


def check(buf, off, lens, flags=0, ctx=""):
    from pebble_amd.batch import BlockBatch, decode
    hide = flags & N.PBL_ROW_HIDE_OBSOLETE
    o = oracle.decode_batch(buf, off, lens, 0, None, flags) if hide else oracle.rowblk_decode_batch(buf, off, lens, flags)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags | POOL)).to_host()
    assert_same(g, o, ctx)
    return g, o


def special_blocks():
    """One block of every kind that leaves the fast path or the early release."""
    rng = random.Random(5)

    def rows(ri, n, vl=20, kl=12):
        w = Writer(ri)
        for k in range(n):
            w.add(b"k%0*d" % (kl - 1, k), make_trailer(9 + k, 1), bytes([k & 255]) * vl)
        return w.finish()

    cases = dict(header_cases())
    big = blocks_of(*gen_row_blocks(8, 1, 40000, 16, 16, 100)[:3])[0]
    bad_restarts = bytearray(rows(16, 60))
    bad_restarts[-8:-4] = (0x7fffff00).to_bytes(4, "little")  # a restart offset past the block
    out = {
        "over": rows(40, 90),                 # runs longer than the 16 parked entries: the late release
        "over_tail": rows(17, 70, 3),
        "many": rows(1, 700, 1, 10),          # more entries than a slot holds: the general walk
        "vlen3": cases["vlen 3 bytes"],       # 3-byte header varints: the general walk
        "vlen3_canonical": cases["vlen 3 bytes, canonical (20000)"],
        "big": big,                           # past kMaxFastLen: block_big
        "empty": Writer(16).finish(),
        "nothing": b"",
        "bad_restarts": bytes(bad_restarts),
        "bad_nres": rows(16, 60)[:-4] + (0x00ffffff).to_bytes(4, "little"),  # more restarts than bytes
        "shared_past_prev": cases["shared > previous key"],
        "first_shared": cases["first entry shared != 0"],
        "mvcc": mvcc_block(rng, 120, 16, False, True),
        "mvcc_vp": mvcc_block(rng, 120, 16, True, True),
    }
    assert len(out["big"]) > 32768 and len(out["many"]) <= 32768
    return out


@pytest.fixture(scope="module")
def uni_blocks():
    """Two shapes of small uniform blocks: one emit step per block (100-B
    values) and several (4-B values: well past 128 KVs per block)."""
    a = blocks_of(*uniform(11, 256, 4096, 16, 100)[:3])
    b = blocks_of(*uniform(12, 256, 4096, 16, 4)[:3])
    return a, b


@pytest.fixture(scope="module")
def interleaved(uni_blocks):
    """About 8 Ki blocks with a special block every few uniform ones, in an
    order that puts every kind before and after every other."""
    a, b = uni_blocks
    sp = list(special_blocks().items())
    rng = random.Random(17)
    blocks, kinds = [], []
    for i in range(NB):
        if i % 5 == 3 or (i % 97) in (10, 11, 12):  # singly, and three in a row
            k, blk = sp[rng.randrange(len(sp))]
            # (the 40 KB block: often enough to be current and prefetched, rare enough to stay quick)
            if k in ("big", "many", "vlen3_canonical") and rng.random() < 0.8:
                k, blk = sp[0]
            blocks.append(blk)
            kinds.append(k)
        else:
            blocks.append((a if i % 2 else b)[rng.randrange(256)])
            kinds.append("uni")
    assert {k for k, _ in sp} <= set(kinds)
    return pack(blocks)


def test_uniform_small_blocks(uni_blocks):
    a, b = uni_blocks
    rng = random.Random(3)
    for name, pool in (("one step", a), ("several steps", b)):
        blocks = [pool[rng.randrange(256)] for _ in range(NB)]
        g, o = check(*pack(blocks), 0, f"uniform {name}")
        assert g["status_mask"] == 0 and g["n_kv"] > 64 * NB // 4
    assert max(oracle.rowblk_decode_batch(*pack(b[:8]), 0)["blk_kv_base"][1:] -
               oracle.rowblk_decode_batch(*pack(b[:8]), 0)["blk_kv_base"][:-1]) > 130  # three steps or more
    for n in (1, 3):  # nothing to prefetch
        check(*pack(a[:n]), 0, f"uniform n={n}")
        check(*pack(b[:n]), 0, f"uniform n={n}")


def test_every_block_kind_as_current_and_prefetched(interleaved):
    g, o = check(*interleaved, 0, "interleaved")
    assert g["n_bad_blocks"] > 100 and g["n_slow_blocks"] > 100
    assert (o["blk_status"] == N.PBL_CORRUPT_BOUNDS).any()


@pytest.mark.parametrize("flags", [N.PBL_ROW_VALUE_PREFIX, N.PBL_ROW_HIDE_OBSOLETE, N.PBL_ROW_RAW_KEYS,
                                   N.PBL_ROW_VALUE_PREFIX | N.PBL_ROW_HIDE_OBSOLETE])
def test_flags(interleaved, uni_blocks, flags):
    """Value prefixes keep the stage through the metadata pass everywhere."""
    check(*interleaved, flags, f"interleaved flags={flags:#x}")
    a, b = uni_blocks
    check(*pack((a[:64] + b[:64]) * 40), flags, f"uniform flags={flags:#x}")


def test_mixed_batch_row_ids():
    """Even ids row, odd ids crdb1 colblk: the prefetch reads its ticket's block id from the id list."""
    from pebble_amd.batch import BlockBatch, decode
    from pebble_amd.colblk import gen_col_blocks
    rows = blocks_of(*uniform(21, 128, 4096, 16, 40)[:3])
    cols = blocks_of(*gen_col_blocks(21, 128, 4096)[:3])
    rng = random.Random(22)
    n = NB - 1
    blocks = [(rows if i % 2 == 0 else cols)[rng.randrange(128)] for i in range(n)]
    bf = np.array([N.PBL_FMT_ROW if i % 2 == 0 else N.PBL_FMT_COL_CRDB1 for i in range(n)], np.uint8)
    buf, off, lens = pack(blocks)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, bf)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0, block_format=bf)).to_host()
    assert_same(g, o, "mixed")
    assert g["status_mask"] == 0


def test_overflowing_capacities(uni_blocks):
    """The KV capacity one short of the first 100 blocks' KVs: block 99 and
    every later block reports PBL_OVERFLOW (its emit returns before the
    prefetch point), the sizes stay exact and the blocks before are written."""
    import torch
    from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode_into
    a, b = uni_blocks
    rng = random.Random(31)
    buf, off, lens = pack([(a if i % 2 else b)[rng.randrange(256)] for i in range(NB)])
    o = oracle.rowblk_decode_batch(buf, off, lens, 0)
    assert o["status_mask"] == 0
    kvb = o["blk_kv_base"]
    cap = Capacity(kv=int(kvb[100]) - 1, key=o["key_bytes_total"], val=o["val_bytes_total"], rst=o["n_restarts"])
    batch = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, POOL)
    out = DecodedBatch.allocate(NB, cap, "cuda")
    decode_into(batch, out)
    torch.cuda.synchronize()
    t = out.read_totals()
    want = np.where(kvb[1:] > cap.kv, N.PBL_OVERFLOW, N.PBL_OK).astype(np.uint32)
    assert want[98] == N.PBL_OK and (want[99:] == N.PBL_OVERFLOW).all()
    assert np.array_equal(out.blk_status.cpu().numpy().view(np.uint32), want)
    assert (t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"])
    assert t.status_mask == 1 << N.PBL_OVERFLOW and t.n_bad_blocks == NB - 99
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base"):
        assert np.array_equal(getattr(out, k).cpu().numpy().view(np.uint64), o[k]), k
    n = int(kvb[99])  # the KVs of the blocks that were written
    nk, nv = int(o["blk_key_base"][99]), int(o["blk_val_base"][99])
    assert np.array_equal(out.trailer[:n].cpu().numpy().view(np.uint64), o["trailer"][:n])
    assert np.array_equal(out.key_off[:n + 99].cpu().numpy().view(np.uint32), o["key_off"][:n + 99])
    assert np.array_equal(out.key_bytes[:nk].cpu().numpy(), o["key_bytes"][:nk])
    assert np.array_equal(out.val_bytes[:nv].cpu().numpy(), o["val_bytes"][:nv])


def test_size_pass(interleaved):
    """pbl_size_batch: every emit returns early; statuses, bases and totals are the oracle's."""
    import torch
    from pebble_amd.batch import BlockBatch, size_batch
    buf, off, lens = interleaved
    o = oracle.rowblk_decode_batch(buf, off, lens, 0)
    s = size_batch(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, POOL))
    torch.cuda.synchronize()
    t = s.read_totals()
    assert (t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts, t.status_mask, t.n_bad_blocks) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"], o["status_mask"], o["n_bad_blocks"])
    assert np.array_equal(s.blk_status.cpu().numpy().view(np.uint32), o["blk_status"])
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base"):
        assert np.array_equal(getattr(s, k).cpu().numpy().view(np.uint64), o[k]), k
