"""The staging-pool row kernel's two-level look-back (common.hip.h, PBL_LB_L2):
block ids are grouped into chunks of 64, the wave that resolves a chunk's last
block publishes the chunk's summed aggregate and later its inclusive prefix,
and a resolve adds whole chunks where their records are there instead of
walking their 64 block records.  A chunk record is never waited for: a chunk
with a wide aggregate, or whose last block another kernel resolves (a colblk
block of a mixed batch), publishes none and costs the walk.

The library ships with PBL_LB_L2 0 (the two-level form measured no gain beyond
the parents' spread) and with the pool kernel's own window counts (two windows
in a resolve's first round trip, one in every later one); the cases are the
same for either form: the block counts around the chunk and window edges, the
chunks that must not publish, the kernels whose look-back is unchanged over
the grown workspace.  They passed on builds of both forms.

Every case is compared with the oracle, bit-exact on every output array.
Blocks are 1-2 KiB (a few restart runs); the block bases are the look-back's
result, so a wrong sum shows in blk_*_base and in every array placed by them."""
import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.colblk import gen_col_blocks
from pebble_amd.rowblk import Writer, gen_row_blocks
from test_pool_emit_steps_gpu import block
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
POOL = N.PBL_KERNEL_POOL
HIDE = N.PBL_ROW_HIDE_OBSOLETE
CHUNK = 64
# around the chunk (64) and window (128) edges; 4096 +- 1 (64 chunks: one chunk
# window exactly); 8192 is more than twice the resident waves, so waves take
# further tickets and the steady state occurs
COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 4095, 4096, 4097, 8192]


@pytest.fixture(scope="module")
def small_blocks():
    """16 distinct blocks of 20..50 KVs, every 4th KV obsolete."""
    return [block([(16, 0, 40, 17)[k % 4] for k in range(20 + 2 * i)], ri=8, obsolete=4, seed=i) for i in range(16)]


def batch_of(small, n, start=0):
    return [small[(start + 7 * i) % len(small)] for i in range(n)]


def check_row(blocks, flags=0, ctx=""):
    from pebble_amd.batch import BlockBatch, decode
    buf, off, lens = pack(blocks, 1)
    o = oracle.decode_batch(buf, off, lens, 0, None, flags) if flags & HIDE else oracle.rowblk_decode_batch(buf, off, lens, flags)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags)).to_host()
    assert_same(g, o, ctx)
    return g, o


@pytest.mark.parametrize("hide", [0, HIDE])
@pytest.mark.parametrize("n", COUNTS)
def test_block_counts_around_chunk_and_window_edges(small_blocks, n, hide):
    g, o = check_row(batch_of(small_blocks, n, n), POOL | hide, f"{n} blocks, hide {hide}")
    assert g["status_mask"] == 0 and g["n_kv"] == o["n_kv"] > 0


@pytest.mark.parametrize("pos", [0, 31, 62, 63])
def test_chunk_with_a_wide_aggregate_publishes_nothing(small_blocks, pos):
    """One block with more value bytes than the packed aggregate holds (a Wide
    record) in the second of four chunks: at the chunk's last position the
    block itself is the publisher."""
    buf, off, lens, _ = gen_row_blocks(7, 1, 300000, 16, 16, 3000)
    wide = bytes(buf[int(off[0]):int(off[0]) + int(lens[0])])
    blocks = batch_of(small_blocks, 4 * CHUNK, pos)
    at = CHUNK + pos
    blocks[at] = wide
    g, o = check_row(blocks, POOL, f"wide at {pos}")
    assert int(o["blk_val_base"][at + 1] - o["blk_val_base"][at]) > 1 << 18
    assert g["status_mask"] == 0


@pytest.mark.parametrize("pos", [0, 63])
def test_corrupt_and_empty_blocks_at_chunk_edges(small_blocks, pos):
    """Zero aggregates: a block cut short (a non-OK status) and an empty block
    (status OK), each at the chunk position `pos` of two different chunks."""
    blocks = batch_of(small_blocks, 4 * CHUNK, 3 + pos)
    blocks[CHUNK + pos] = blocks[CHUNK + pos][:100]
    blocks[2 * CHUNK + pos] = Writer(16).finish()
    g, o = check_row(blocks, POOL, f"corrupt at {pos}")
    assert o["blk_status"][CHUNK + pos] != N.PBL_OK and g["n_bad_blocks"] == 1
    assert o["blk_kv_base"][2 * CHUNK + pos + 1] == o["blk_kv_base"][2 * CHUNK + pos]


def test_block_past_the_stage_at_a_chunks_last_position(small_blocks):
    """A block over 32 KiB: the sizes kernel publishes its aggregate before the
    launch and block_big resolves it, here as its chunk's publisher."""
    buf, off, lens, _ = gen_row_blocks(6, 1, 40000, 16, 16, 100)
    big = bytes(buf[int(off[0]):int(off[0]) + int(lens[0])])
    assert len(big) > 32768
    blocks = batch_of(small_blocks, 3 * CHUNK + 1, 5)
    blocks[2 * CHUNK - 1] = big
    g, o = check_row(blocks, POOL, "big block at a chunk tail")
    assert g["status_mask"] == 0 and g["n_slow_blocks"] == 1


@pytest.fixture(scope="module")
def col_blocks():
    cb, co, cl, _ = gen_col_blocks(11, 8, 2048)
    return [bytes(cb[int(co[i]):int(co[i]) + int(cl[i])]) for i in range(8)]


@pytest.mark.parametrize("n", [130, 257])
def test_mixed_batch_whose_chunk_tails_are_colblk(small_blocks, col_blocks, n):
    """The colblk blocks' records come from the colblk size kernel and their
    resolves from the colblk pipeline: the chunks' last blocks are all colblk,
    so no chunk record is ever written and the row kernel walks as before."""
    from pebble_amd.batch import BlockBatch, decode
    R, C = N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1
    fmts = [C if i % CHUNK == CHUNK - 1 or i % 5 == 2 else R for i in range(n)]
    rows = batch_of(small_blocks, n, n)
    blocks = [col_blocks[i % len(col_blocks)] if f == C else rows[i] for i, f in enumerate(fmts)]
    buf, off, lens = pack(blocks, 8)
    bf = np.array(fmts, np.uint8)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW, bf)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0, block_format=bf)).to_host()
    assert_same(g, o, f"mixed {n}")
    assert g["status_mask"] == 0


@pytest.mark.parametrize("n", [130, 257])
def test_kernels_on_the_one_level_form_are_unchanged(small_blocks, col_blocks, n):
    """A PBL_BATCH_VARLEN row batch (the two-pass wave form) and a colblk batch:
    their look-backs keep the one-level form over the grown workspace."""
    from pebble_amd.batch import BlockBatch, decode
    check_row(batch_of(small_blocks, n, n), N.PBL_BATCH_VARLEN, f"varlen {n}")
    blocks = [col_blocks[(3 * i) % len(col_blocks)] for i in range(n)]
    buf, off, lens = pack(blocks, 8)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_COL_CRDB1, None)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_COL_CRDB1, 0)).to_host()
    assert_same(g, o, f"colblk {n}")
