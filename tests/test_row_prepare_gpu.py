"""The pool path's two launches -- row_prepare_kernel (the look-back state, the
workspace header and the totals cleared per window of block ids, the blocks
past the 32 KiB stage sized) and the staging-pool kernel (which sizes the
blocks the prepare launch left with a stage as the key buffer, and writes a
big block whose key outgrows the slot with a stage taken again) -- against the
oracle, bit-exact on every output array.

Every case runs on a workspace, totals and per-block outputs filled with 0xFF
bytes, twice into the same outputs (dirtied again in between): a missed clear
shows as a wrong array or as PBL_TIMEOUT.  Workspaces come without key spill
slots (the row kernel's own second tier and staged write walk) and with them
(pbl_workspace_bytes_for: the long-key kernels between the two launches)."""
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, gen_row_blocks, make_trailer
from test_mixed_gpu import _big_row_block, pool
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
R, C = N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1
COUNTS = [1, 7, 8, 9, 63, 64, 65, 129, 4097]  # around the windows of 8 ids and the chunks of 64


def run(buf, off, lens, flags=0, bf=None, slots=False, ctx=""):
    """Decode into dirty outputs, twice, and compare with the oracle.  A row
    batch is forced onto the pool kernel (lengths that vary would otherwise
    route it to the two-pass form, which keeps its memsets)."""
    import torch
    from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode_into
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, bf, flags)
    kern = 0 if bf is not None else N.PBL_KERNEL_POOL
    b = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags | kern, block_format=bf)
    cap = Capacity(kv=o["n_kv"], key=o["key_bytes_total"], val=o["val_bytes_total"], rst=o["n_restarts"])
    out = DecodedBatch.allocate(b.n_blocks, cap, "cuda", max_block_len=b.max_block_len if slots else 0)
    # (slots come only with a block past 32 KiB)
    assert (slots and b.max_block_len > 32768) == (out.workspace.numel() > N.lib().pbl_workspace_bytes(b.n_blocks))
    for rnd in range(2):
        for t in (out.workspace, out.totals, out.blk_status, out.blk_kv_base, out.blk_key_base, out.blk_val_base,
                  out.blk_rst_base):
            t.view(torch.uint8).fill_(0xFF)
        decode_into(b, out)
        torch.cuda.synchronize()
        g = out.to_host()
        assert not g["status_mask"] & (1 << N.PBL_TIMEOUT), f"{ctx} round {rnd}: PBL_TIMEOUT"
        assert_same(g, o, f"{ctx} slots={slots} round {rnd}")
    return g


@pytest.fixture(scope="module")
def small4k():
    """4097 small blocks (4 KiB, restart interval 16), plain and with every 4th KV obsolete."""
    return {hide: gen_row_blocks(11, max(COUNTS), 4096, 16, 16, 100, obsolete_every=4 if hide else 0)
            for hide in (False, True)}


@pytest.mark.parametrize("hide", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_counts_around_the_window_edges(small4k, n, hide):
    buf, off, lens, _ = small4k[hide]
    end = int(off[n - 1]) + int(lens[n - 1])
    sub = np.concatenate([buf[:end], np.zeros(16, np.uint8)])
    g = run(sub, off[:n], lens[:n], N.PBL_ROW_HIDE_OBSOLETE if hide else 0, ctx=f"n={n} hide={hide}")
    assert g["status_mask"] == 0 and g["n_kv"] > 0


def small_blocks(seed, n):
    buf, off, lens, _ = gen_row_blocks(seed, n, 4096, 16, 16, 100)
    return [bytes(buf[int(o): int(o) + int(l)]) for o, l in zip(off, lens)]


def block_40k(rng):
    blk = _big_row_block(rng, n=5, vlen=8000)
    assert 32768 < len(blk) <= 41 * 1024
    return blk


def block_long_key(rng, i=0):
    """48 KiB with one 12 KB key: past the prepare launch's 8 KiB buffer (the
    row kernel sizes it, with a stage) and past the slot (the row kernel writes
    it with a stage taken again)."""
    w = Writer(rng.choice([1, 16]))
    w.add(b"a%07d" % i, make_trailer(9, 1), bytes([1]) * 12400)
    w.add(b"b" + bytes(rng.randrange(256) for _ in range(12000)), make_trailer(8, 1), bytes([2]) * 12400)
    w.add(b"c%07d" % i, make_trailer(7, 1), bytes([3]) * 12400)
    blk = w.finish()
    assert 48 * 1024 <= len(blk) < 49 * 1024
    return blk


@pytest.mark.parametrize("slots", [False, True])
def test_big_blocks_at_the_ends_and_at_a_window_edge(slots):
    rng = random.Random(5)
    blocks = small_blocks(12, 20)
    for at in (0, 7, 8, len(blocks) - 1):
        blocks[at] = block_40k(rng)
    for flags in (0, N.PBL_ROW_HIDE_OBSOLETE):
        g = run(*pack(blocks), flags, slots=slots, ctx=f"40 KiB blocks flags={flags}")
        assert g["status_mask"] == 0 and g["n_slow_blocks"] == 4


@pytest.mark.parametrize("slots", [False, True])
def test_a_block_for_the_second_tier(slots):
    rng = random.Random(6)
    blocks = small_blocks(13, 11)
    blocks[4] = block_long_key(rng)
    blocks[5] = block_40k(rng)
    g = run(*pack(blocks), 0, slots=slots, ctx="12 KB key")
    assert g["status_mask"] == 0
    # alone in its batch, and as block 0 and as the last block
    run(*pack([block_long_key(rng)]), 0, slots=slots, ctx="12 KB key alone")
    run(*pack([block_long_key(rng, 1)] + blocks[:9] + [block_long_key(rng, 2)]), 0, slots=slots, ctx="12 KB key at the ends")


def bad_big_blocks(rng):
    bad = []
    b = bytearray(_big_row_block(rng)); b[-4:] = (0).to_bytes(4, "little"); bad.append(bytes(b))         # no restarts
    b = bytearray(_big_row_block(rng)); b[-4:] = (1 << 20).to_bytes(4, "little"); bad.append(bytes(b))   # table > block
    b = bytearray(_big_row_block(rng)); b[0] = 3; bad.append(bytes(b))                                   # shared != 0
    b = bytearray(_big_row_block(rng)); b[1] = 4; bad.append(bytes(b))                                   # key < 8 bytes
    b = bytearray(block_long_key(rng)); b[-4:] = (0).to_bytes(4, "little"); bad.append(bytes(b))         # the same, long key
    return bad


@pytest.mark.parametrize("slots", [False, True])
def test_big_blocks_failing_the_init_checks(slots):
    rng = random.Random(7)
    bad = bad_big_blocks(rng)
    small = small_blocks(14, 12)
    blocks = [bad[0]] + small[:6] + [bad[1], bad[2], block_40k(rng)] + small[6:] + [bad[3], bad[4]]
    for flags in (0, N.PBL_ROW_HIDE_OBSOLETE):
        g = run(*pack(blocks), flags, slots=slots, ctx=f"bad big blocks flags={flags}")
        assert g["n_bad_blocks"] == len(bad)


def test_more_big_blocks_in_a_row_than_a_cu_has_stages():
    """Every wave of a workgroup draws a block whose write walk takes a stage
    again (8 waves, 3 stages), for several rounds, among 40 KiB blocks."""
    rng = random.Random(8)
    lk, b40 = block_long_key(rng), block_40k(rng)
    blocks = small_blocks(15, 3) + [lk] * 30 + [b40, lk] * 5 + small_blocks(16, 5) + [lk] * 10
    g = run(*pack(blocks), 0, ctx="long-key blocks in a row")
    assert g["status_mask"] == 0 and g["n_slow_blocks"] == 50


@pytest.mark.parametrize("slots", [False, True])
def test_mixed_batches(slots):
    """The same ingredients in a mixed batch: the prepare launch sizes the big
    row blocks only, and the format split writes the header after it."""
    rng = random.Random(9)
    rows, cols = pool(10, 12, 12, 4096)
    bad = bad_big_blocks(rng)
    blocks = [block_40k(rng), cols[0]] + rows[:5] + [block_long_key(rng), block_40k(rng)] + cols[1:7] + \
        [bad[0], bad[4]] + rows[5:] + cols[7:] + [block_long_key(rng, 1)]
    fmts = [R, C] + [R] * 5 + [R, R] + [C] * 6 + [R, R] + [R] * 7 + [C] * 5 + [R]
    bf = np.array(fmts, np.uint8)
    for flags in (0, N.PBL_ROW_HIDE_OBSOLETE):
        g = run(*pack(blocks), flags, bf=bf, slots=slots, ctx=f"mixed flags={flags}")
        assert g["n_bad_blocks"] == 2
    # all colblk but one big row block; counts around the window edges
    for n in (7, 8, 9, 65):
        bl = [cols[i % len(cols)] if i % 3 else rows[i % len(rows)] for i in range(n)]
        fm = np.array([C if i % 3 else R for i in range(n)], np.uint8)
        run(*pack(bl), 0, bf=fm, slots=slots, ctx=f"mixed n={n}")


@pytest.mark.parametrize("mixed", [False, True])
def test_overflow_retry_and_size_pass(mixed):
    """pbl_size_batch and the overflow retry (test_overflow_and_size_pass's
    route) over a batch with big blocks of every kind: the same bases, totals
    and arrays."""
    import torch
    from pebble_amd.batch import BlockBatch, Capacity, decode, size_batch
    rng = random.Random(10)
    rows, cols = pool(11, 10, 10, 4096)
    bad = bad_big_blocks(rng)
    blocks = [block_long_key(rng)] + rows[:9] + [block_40k(rng), bad[1]] + (cols if mixed else rows) + [block_40k(rng)]
    fmts = [R] * 12 + [C if mixed else R] * 10 + [R]
    bf = np.array(fmts, np.uint8) if mixed else None
    buf, off, lens = pack(blocks)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, bf, 0)
    b = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0 if mixed else N.PBL_KERNEL_POOL, block_format=bf)
    assert_same(decode(b, cap=Capacity(kv=10, key=10, val=10, rst=10)).to_host(), o, "overflow retry")
    assert_same(decode(b, exact=True).to_host(), o, "size pass, then decode")
    b.max_block_len = 0  # (a workspace without key spill slots)
    assert_same(decode(b, cap=Capacity(kv=10, key=10, val=10, rst=10)).to_host(), o, "overflow retry, no slots")
    s = size_batch(b)
    torch.cuda.synchronize()
    t = s.read_totals()
    assert (t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"])
    assert t.n_bad_blocks == 1
    assert np.array_equal(s.blk_kv_base.cpu().numpy().view(np.uint64), o["blk_kv_base"])
    assert np.array_equal(s.blk_val_base.cpu().numpy().view(np.uint64), o["blk_val_base"])
    assert np.array_equal(s.blk_status.cpu().numpy().view(np.uint32), o["blk_status"])
