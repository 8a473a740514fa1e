"""The zstd decoders on the device over every format feature zstd.hip claims:
facebook/zstd frames with Huffman literals and the frames tests/zstdutil.py
assembles (direct weights, forced size formats, RLE literals, RLE / FSE /
repeat tables, repeat offsets, every match-copy branch, the 3-byte sequence
count, every frame-header form, the content checksum), each sent down the
batch path, zstd_kernel's LDS route and its global-memory route by
zstdutil's route wrappers; the batch path running out of its sequence area;
and damaged frames, on which the three routes must agree with the oracle.

tests/test_zstd_forms.py holds the same frames to facebook/zstd and the oracle
on the CPU, and the corpus to its coverage floor.  Every comparison is exact."""
import random

import numpy as np
import pytest

import oracle
import zstdutil as Z
from pebble_amd import _native as N
from pebble_amd.physical import PhysBatch, decompress

pytestmark = pytest.mark.gpu
ZSTD, SNAPPY, RAW = 7, 1, 0


def device(blocks, inds=None, seed=0):
    """decompress() of Pebble blocks at ragged input offsets: [(status, bytes)]."""
    rng = random.Random(seed)
    buf, off, lens = bytearray(), [], []
    for i, bk in enumerate(blocks):
        buf += bytes(rng.randrange(0, 8))
        off.append(len(buf))
        lens.append(len(bk))
        buf += bytes(bk) + bytes([inds[i] if inds else ZSTD]) + bytes(4)
    buf += bytes(16)
    bb, st = decompress(PhysBatch.from_host(np.frombuffer(bytes(buf), np.uint8), off, lens))
    out, bo, bl = bb.blocks.cpu().numpy(), bb.block_off.cpu().numpy(), bb.block_len.cpu().numpy()
    return [(int(st[i]), bytes(out[bo[i]: bo[i] + bl[i]])) for i in range(len(blocks))]


def check_all_routes(cases, oracle_every=7):
    blocks = [wrap(c.frame, len(c.want)) for c in cases for wrap in Z.ROUTES]
    got = device(blocks)
    for k, (st, data) in enumerate(got):
        c, route = cases[k // 3], Z.ROUTES[k % 3].__name__
        assert st == 0, (c.name, route, st)
        assert data == c.want, (c.name, route)
        if k % oracle_every == 0:
            assert oracle.zstd_block(blocks[k]) == c.want, (c.name, route)


def test_library_huffman_frames_on_all_routes():
    check_all_routes(Z.library_frames())


def test_assembled_forms_on_all_routes():
    check_all_routes(Z.assembled_forms(), oracle_every=1)


def test_rejected_frames_on_all_routes():
    """A bad content checksum, rep0 - 1 == 0, an empty fourth stream, a first
    block that repeats a table or a tree (alone, and behind a frame that set
    them, which a decoder carrying state from frame to frame would decode):
    corrupt; a non-zero dictionary ID: unsupported -- on the batch path's
    planner and both zstd_kernel routes."""
    cases = Z.rejected_forms()
    got = device([wrap(c.frame, c.want) for c in cases for wrap in Z.ROUTES])
    for k, (st, data) in enumerate(got):
        c = cases[k // 3]
        want = N.PBL_UNSUPPORTED if c.feature == "unsupported" else N.PBL_CORRUPT_COMPRESSION
        assert (st, data) == (want, b""), (c.name, Z.ROUTES[k % 3].__name__)


def test_library_checksum_one_bit_off_on_all_routes():
    rng = random.Random(41)
    good, bad, want = [], [], []
    for n in (40, 1000, 20000, 36864):
        data = Z.letters(rng, n)
        f = Z.compress(data, 3, checksum=True)
        b = bytearray(f)
        b[-1 - rng.randrange(4)] ^= 1 << rng.randrange(8)
        good += [w(f, n) for w in Z.ROUTES]
        bad += [w(bytes(b), n) for w in Z.ROUTES]
        want += [data] * 3
    got = device(good + bad)
    assert got[:len(good)] == [(0, d) for d in want]
    assert got[len(good):] == [(N.PBL_CORRUPT_COMPRESSION, b"")] * len(bad)


def test_multi_block_frames():
    """Only zstd_kernel takes them: the 140,000-byte library frames (treeless
    literals, repeat tables; global route) and the assembled two-block frames
    (LDS route as they are, global route behind the pad)."""
    cases = Z.multi_block_frames() + [c for c in Z.assembled_forms() if "frame_multi_block" in c.feature]
    assert len(cases) >= 5
    blocks = [Z.as_is(c.frame, len(c.want)) for c in cases] + [Z.skippable_pad(c.frame, len(c.want)) for c in cases[2:]]
    want = [c.want for c in cases] + [c.want for c in cases[2:]]
    assert device(blocks) == [(0, w) for w in want]
    assert oracle.zstd_block(blocks[0]) == want[0]


def test_three_byte_sequence_count():
    """0x7F00 and 0x7F00 + 200 sequences in one block each (about 130 KB
    decoded: the global route), the only reach of that branch."""
    cases = Z.long_count_frames()
    got = device([Z.as_is(c.frame, len(c.want)) for c in cases])
    assert got == [(0, c.want) for c in cases]


def test_sequence_area_exhaustion():
    """64 text blocks of more than 4096 sequences each: the batch path's
    sequence area (kSeqPerBlock a block on average) runs out part way, in an
    order its atomic counter decides, and zstd_kernel takes the rest."""
    batch = Z.exhaustion_batch()
    nseq = [Z.first_block_nseq(f)[0] for f, _ in batch]
    assert sum(nseq) > 64 * Z.SEQ_PER_BLOCK and Z.min_fallbacks(nseq, 64) >= 3
    got = device([Z.as_is(f, len(d)) for f, d in batch])
    assert [st for st, _ in got] == [0] * 64
    assert [data == d for (_, data), (_, d) in zip(got, batch)] == [True] * 64


def test_sequence_area_exhaustion_among_other_codecs():
    """The area is sized over every block of the batch, so the 22 snappy and
    raw blocks widen it: the 88 zstd blocks (24 of them dense, assembled) still
    hold more sequences than all 110 blocks' share, and at least 4 of them
    fall to zstd_kernel with other codecs' entries between theirs."""
    batch = Z.exhaustion_batch_mixed()
    nseq = Z.batch_nseq(batch)
    assert {ind for _, ind, _ in batch} == {ZSTD, SNAPPY, RAW} and len(nseq) == 88
    assert sum(nseq) > len(batch) * Z.SEQ_PER_BLOCK and Z.min_fallbacks(nseq, len(batch)) >= 4
    got = device([bk for bk, _, _ in batch], [ind for _, ind, _ in batch], seed=1)
    assert [st for st, _ in got] == [0] * len(batch)
    assert [data == d for (_, data), (_, _, d) in zip(got, batch)] == [True] * len(batch)


def test_damaged_frames_agree_on_all_routes_and_with_the_oracle():
    cases = Z.damaged(random.Random(42), Z.assembled_forms() + Z.library_frames(), 84)
    got = device([wrap(f, n) for _, f, n in cases for wrap in Z.ROUTES])
    errors = 0
    for k, (name, f, n) in enumerate(cases):
        want = oracle.zstd_block(Z.as_is(f, n))
        three = got[3 * k: 3 * k + 3]
        if isinstance(want, int):
            errors += 1
            assert all(st in (N.PBL_CORRUPT_COMPRESSION, N.PBL_UNSUPPORTED) and data == b"" for st, data in three), (name, three)
        else:
            assert three == [(0, want)] * 3, name
    assert 20 < errors < len(cases)   # both outcomes occur
