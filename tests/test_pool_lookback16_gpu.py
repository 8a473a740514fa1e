"""The staging-pool row kernel's look-back records as single 16-byte accesses
(common.hip.h, kLbV16 / kLbSt16; rowblk_pool.hip.h, PBL_LB_V16,
PBL_POOL_LB_ST16, PBL_POOL_LB_LATER_LANES): a window of 64 predecessor records
is one 16-byte load per lane, a packed prefix one 16-byte store, and a
resolve's first later round trip loads only the 16 records below where the
first trip ended (a trip after a partial one that found no prefix is a full
window again).  Every other kernel keeps the 8-byte accesses on the same
records, so the two forms meet in one workspace: records written with 8-byte
stores (the colblk size kernel's, the big-block sizes kernel's, every
aggregate) are read with 16-byte loads and the other way round.

The cases: the block counts around every window edge (64, 128, 192) and
partial-window edge (16 past a window: 144, 160), one past the resident waves
(2049) and the steady state (8192); records published by other kernels; a
Wide aggregate (four more per-lane loads inside a window, whole or partial);
zero aggregates; the kernels that keep the 8-byte form.  The walk's length
depends on timing, so this file and test_pool_lookback_gpu.py were run against
two builds and passed on both: the committed default, and a variant with
-DPBL_POOL_LB_WIN=1 -DPBL_POOL_LB_LATER_LANES=16, in which every resolve that
meets its prefix more than 64 records back alternates partial and full trips.
The PfxWide path (inclusive prefixes too wide to pack) needs >= 1 GiB of key
bytes in one batch and is code the 16-byte forms do not touch: it stays
uncovered here.

Every case is compared with the oracle, bit-exact on every output array: the
block bases are the look-back's result, so a wrong sum shows in blk_*_base and
in every array placed by them."""
import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, gen_row_blocks
from test_pool_emit_steps_gpu import block  # noqa: F401  (small_blocks builds on it)
from test_pool_lookback_gpu import batch_of, check_row, col_blocks, small_blocks  # noqa: F401
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
POOL = N.PBL_KERNEL_POOL
HIDE = N.PBL_ROW_HIDE_OBSOLETE
COUNTS = [1, 2, 15, 16, 17, 64, 65, 128, 129, 130, 143, 144, 145, 160, 161, 192, 193, 2049, 8192]
# records back from the batch's last block: the last record of the first trip's
# two windows, the first of a later trip, and the last of a 16-lane partial one
BACK = [127, 128, 143]
N_BATCH = 300


@pytest.mark.parametrize("hide", [0, HIDE])
@pytest.mark.parametrize("n", COUNTS)
def test_block_counts_around_window_and_partial_window_edges(small_blocks, n, hide):
    g, o = check_row(batch_of(small_blocks, n, n), POOL | hide, f"{n} blocks, hide {hide}")
    assert g["status_mask"] == 0 and g["n_kv"] == o["n_kv"] > 0


@pytest.mark.parametrize("n", [130, 257])
def test_mixed_batch_records_of_the_colblk_size_kernel(small_blocks, col_blocks, n):
    """The colblk blocks' records are written by the colblk size kernel with
    8-byte stores and read by the row kernel's 16-byte loads; the colblk
    pipeline reads the row kernel's 16-byte prefix stores with 8-byte loads."""
    from pebble_amd.batch import BlockBatch, decode
    R, C = N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1
    fmts = [C if i % 3 == 1 or i % 16 == 15 else R for i in range(n)]
    rows = batch_of(small_blocks, n, n)
    blocks = [col_blocks[i % len(col_blocks)] if f == C else rows[i] for i, f in enumerate(fmts)]
    buf, off, lens = pack(blocks, 8)
    bf = np.array(fmts, np.uint8)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, bf)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0, block_format=bf)).to_host()
    assert_same(g, o, f"mixed {n}")
    assert g["status_mask"] == 0


@pytest.fixture(scope="module")
def big_block():
    buf, off, lens, _ = gen_row_blocks(6, 1, 40000, 16, 16, 100)
    big = bytes(buf[int(off[0]):int(off[0]) + int(lens[0])])
    assert len(big) > 32768
    return big


@pytest.fixture(scope="module")
def wide_block():
    buf, off, lens, _ = gen_row_blocks(7, 1, 300000, 16, 16, 3000)
    return bytes(buf[int(off[0]):int(off[0]) + int(lens[0])])


@pytest.mark.parametrize("back", BACK)
def test_block_past_the_stage_published_before_the_launch(small_blocks, big_block, back):
    """A block over 32 KiB: the sizes kernel publishes its aggregate with an
    8-byte store before the launch, and block_big resolves it with this
    kernel's 16-byte form."""
    blocks = batch_of(small_blocks, N_BATCH, back)
    at = N_BATCH - 1 - back
    blocks[at] = big_block
    g, o = check_row(blocks, POOL, f"big block {back} back")
    assert g["status_mask"] == 0 and g["n_slow_blocks"] == 1


@pytest.mark.parametrize("back", BACK)
def test_wide_aggregate_inside_a_window(small_blocks, wide_block, back):
    """More value bytes than the packed aggregate holds: a Wide record, whose
    four counts a lane of the window fetches on its own (lb_fetch4)."""
    blocks = batch_of(small_blocks, N_BATCH, back + 1)
    at = N_BATCH - 1 - back
    blocks[at] = wide_block
    g, o = check_row(blocks, POOL, f"wide {back} back")
    assert int(o["blk_val_base"][at + 1] - o["blk_val_base"][at]) >= 1 << 18
    assert g["status_mask"] == 0


@pytest.mark.parametrize("pos", [128, 144])
def test_corrupt_and_empty_blocks_at_window_edges(small_blocks, pos):
    """Zero aggregates: a block cut short (a non-OK status) at `pos` and an
    empty block (status OK) 64 further on."""
    blocks = batch_of(small_blocks, N_BATCH, 3 + pos)
    blocks[pos] = blocks[pos][:100]
    blocks[pos + 64] = Writer(16).finish()
    g, o = check_row(blocks, POOL, f"corrupt at {pos}")
    assert o["blk_status"][pos] != N.PBL_OK and g["n_bad_blocks"] == 1
    assert o["blk_kv_base"][pos + 65] == o["blk_kv_base"][pos + 64]


@pytest.mark.parametrize("n", [130, 257])
def test_kernels_that_keep_the_8_byte_form(small_blocks, col_blocks, n):
    """A PBL_BATCH_VARLEN row batch (the two-pass wave form) and a colblk
    batch decode as before."""
    from pebble_amd.batch import BlockBatch, decode
    check_row(batch_of(small_blocks, n, n), N.PBL_BATCH_VARLEN, f"varlen {n}")
    blocks = [col_blocks[(3 * i) % len(col_blocks)] for i in range(n)]
    buf, off, lens = pack(blocks, 8)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_COL_CRDB1, None)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_COL_CRDB1, 0)).to_host()
    assert_same(g, o, f"colblk {n}")
