"""The snappy decoders on the device over every element form snappy.Decode
accepts: the blocks tests/snappyutil.py assembles (1- to 4-byte literal
lengths, non-canonical literal headers, 1-, 2- and 4-byte-offset copies at both
ends of their length range, copies of copies, 1-byte copies, element counts
around a round's queue, the route boundaries), each sent down the walked route
(snappy_walk_kernel + snappy4_kernel), snappy2_kernel's LDS decoder and its
one-lane global-memory decoder by snappyutil's route wrappers -- the front
wrappers put the case's own elements at output offsets past 32768 and 65536;
the blocks snappy.Decode rejects, on every route; damaged blocks, on which the
routes must agree with the oracle and with each other; and what decompress()
never asks of the kernels: output slots packed back to back at every 16-byte
phase, capacity beyond the decoded length, PBL_OVERFLOW, and input blocks at
every 16-byte phase from the first byte of the buffer to its last.

tests/test_snappy_forms.py holds the same blocks to the oracle on the CPU, and
the corpus to its census floor.  Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest
import torch

import oracle
import snappyutil as S
from pebble_amd import _native as N
from pebble_amd.batch import _stream_handle
from pebble_amd.physical import PhysBatch, decompress

pytestmark = pytest.mark.gpu
SNAPPY, MINLZ = 1, 8
CORRUPT = (N.PBL_CORRUPT_COMPRESSION, b"")
CHUNKS = 7   # of the wrapped corpus (a stride coprime to the wrappers per case): under 100 one-lane blocks a test


def device(blocks, ind=SNAPPY, seed=0):
    """decompress() of Pebble blocks at ragged input offsets: [(status, bytes)]."""
    rng = random.Random(seed)
    buf, off, lens = bytearray(), [], []
    for bk in blocks:
        buf += bytes(rng.randrange(0, 8))
        off.append(len(buf))
        lens.append(len(bk))
        buf += bytes(bk) + bytes([ind]) + bytes(4)
    buf += bytes(16)
    bb, st = decompress(PhysBatch.from_host(np.frombuffer(bytes(buf), np.uint8), off, lens))
    out, bo, bl = bb.blocks.cpu().numpy(), bb.block_off.cpu().numpy(), bb.block_len.cpu().numpy()
    return [(int(st[i]), bytes(out[bo[i]: bo[i] + bl[i]])) for i in range(len(blocks))]


def chunk(k):
    blocks = S.wrapped_corpus()[k::CHUNKS]
    assert sum(w.route == "global" for w in blocks) < 100 and {w.route for w in blocks} == set(S.ROUTE_NAMES)
    return blocks


def check_exact(blocks, got):
    assert len(got) == len(blocks)
    for w, (st, data) in zip(blocks, got):
        assert st == 0, (w.name, w.wrapper, w.route, st)
        assert data == w.want, (w.name, w.wrapper, w.route)


@pytest.mark.parametrize("k", range(CHUNKS))
def test_every_form_on_every_route(k):
    blocks = chunk(k)
    check_exact(blocks, device([w.block for w in blocks], seed=k))


@pytest.mark.parametrize("k", range(CHUNKS))
def test_every_form_on_every_route_minlz_indicated(k):
    """Indicator 8 with a first byte other than 0: the Snappy form of a
    MinLZ-indicated block, decoded by the same kernels (a decoded length whose
    varint begins with 0 would read as the MinLZ form)."""
    blocks = [w for w in chunk(k) if w.block[0] != 0]
    assert len(blocks) > 100 and {w.route for w in blocks} == set(S.ROUTE_NAMES)
    check_exact(blocks, device([w.block for w in blocks], ind=MINLZ, seed=10 + k))


def good_neighbours():
    """A few valid blocks of each route, small ones first."""
    by = {r: sorted((w for w in S.wrapped_corpus() if w.route == r), key=lambda w: len(w.want))[:6] for r in S.ROUTE_NAMES}
    return [w for trio in zip(*by.values()) for w in trio]


def test_rejected_blocks_on_every_route():
    """Each of snappy.Decode's ErrCorrupt reasons on the walked, the LDS and
    the global route: corrupt, nothing decoded; the valid blocks between them
    in the batch decode as ever.  (A literal of 2^32 bytes -- fc ff ff ff ff --
    was a literal of none on the global route, whose 32-bit length wrapped.)"""
    bad, good = S.rejected(), good_neighbours()
    assert sum(r.route == "global" for r in bad) < 100
    blocks = []
    for i, r in enumerate(bad):
        blocks += [r.block, good[i % len(good)].block]
    got = device(blocks, seed=3)
    for i, r in enumerate(bad):
        assert got[2 * i] == CORRUPT, (r.name, got[2 * i][0], len(got[2 * i][1]))
        assert got[2 * i + 1] == (0, good[i % len(good)].want), ("after " + r.name)


def test_damaged_blocks_agree_with_the_oracle_and_across_routes():
    """A damaged block as it is (the walked or the LDS route) and behind the
    front pads of the other two routes: each equals the oracle on the same
    bytes; and where the block as it is still decodes, so does it behind
    either pad, to the pad and the same bytes."""
    small = [c for c in S.corpus() if len(c.want) <= 8192]
    cases = S.damaged(random.Random(42), small, 90)
    blocks = [b for _, block in cases for b in (block, S.rewrap_front(block, 32768), S.rewrap_front(block, 65536))]
    routes = [S.route(len(b), S.header(b)[0]) for b in blocks]
    assert set(routes) == set(S.ROUTE_NAMES) and routes[1::3] == ["lds"] * 90 and routes[2::3] == ["global"] * 90
    got = device(blocks, seed=4)
    good = 0
    for k, b in enumerate(blocks):
        want = oracle.snappy_decode(b)
        assert got[k] == (CORRUPT if want is None else (0, want)), (cases[k // 3][0], routes[k])
    for k, (name, block) in enumerate(cases):
        if got[3 * k][0] == 0:
            good += 1
            tail = got[3 * k][1]
            assert [(st, data[-len(tail):] if tail else b"") for st, data in got[3 * k + 1: 3 * k + 3]] == [(0, tail)] * 2, name
    assert 4 * good >= len(cases) and 4 * (len(cases) - good) >= len(cases), good   # both outcomes occur


# ---- pbl_decompress_blocks called directly: the output and the input side ------------------
GUARD, FILL = 64, 0xA5


def direct(pb, caps, out_off, total):
    """pbl_decompress_blocks into a buffer of `total` bytes filled with 0xA5:
    (the whole buffer, out_len, status)."""
    n = len(caps)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    off_t = torch.from_numpy(np.asarray(out_off, np.uint64).view(np.int64)).cuda()
    cap_t = torch.from_numpy(np.asarray(caps, np.uint32).view(np.int32)).cuda()
    lens = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    c = pb.c_struct()
    rc = N.lib().pbl_decompress_blocks(ctypes.byref(c), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(off_t.data_ptr()),
                                       ctypes.c_void_p(cap_t.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
                                       ctypes.c_void_p(st.data_ptr()), _stream_handle(None))
    assert rc == N.PBL_OK
    return out.cpu().numpy(), lens.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


def host_batch(blocks, seed):
    rng = random.Random(seed)
    buf, off, lens = bytearray(), [], []
    for bk in blocks:
        buf += bytes(rng.randrange(0, 8))
        off.append(len(buf))
        lens.append(len(bk))
        buf += bytes(bk) + bytes([SNAPPY]) + bytes(4)
    return PhysBatch.from_host(np.frombuffer(bytes(buf), np.uint8), off, lens)


@pytest.fixture(scope="module")
def packed():
    """About a hundred blocks chosen by census cell, all three routes, with
    literals of 1 to 15 bytes between them sized so that, slots packed with
    cap == D, each route's blocks start at each of the 16 output phases in
    turn; and their device batch."""
    sample = S.sample_by_cell(S.wrapped_corpus(), 2)
    assert sum(w.route == "global" for w in sample) < 100 and {w.route for w in sample} == set(S.ROUTE_NAMES)
    blocks, pos, seen = [], GUARD, {r: 0 for r in S.ROUTE_NAMES}
    for w in sample:
        fill = (seen[w.route] - pos) % 16
        seen[w.route] += 1
        if fill:
            blocks.append(S.Wrapped("filler_%d" % fill, "as_is", "lds", *S.assemble([S.lit(bytes(range(fill)))])))
        blocks.append(w)
        pos += fill + len(w.want)
    assert min(seen.values()) >= 16
    return blocks, host_batch([w.block for w in blocks], 5)


def check_packed(blocks, pb, caps, fits):
    """Slots back to back behind a guard; the whole buffer afterwards is the
    fill, but for the decoded bytes of the blocks that fit."""
    off = GUARD + np.concatenate([[0], np.cumsum(caps)[:-1]])
    total = GUARD + int(np.sum(caps)) + GUARD
    want = np.full(total, FILL, np.uint8)
    for w, o, ok in zip(blocks, off, fits):
        if ok:
            want[o: o + len(w.want)] = np.frombuffer(w.want, np.uint8)
    out, lens, st = direct(pb, caps, off, total)
    assert [int(s) for s in st] == [0 if ok else N.PBL_OVERFLOW for ok in fits]
    assert [int(x) for x in lens] == [len(w.want) if ok else 0 for w, ok in zip(blocks, fits)]
    bad = np.flatnonzero(out != want)
    if len(bad):
        k = int(np.searchsorted(off, bad[0], side="right")) - 1
        raise AssertionError("byte %d differs: block %d (%s %s %s) + %d of %d" % (
            bad[0], k, blocks[max(k, 0)].name, blocks[max(k, 0)].wrapper, blocks[max(k, 0)].route, bad[0] - off[max(k, 0)],
            caps[max(k, 0)]))
    return off


def test_output_slots_packed_at_every_phase(packed):
    """cap == D, no gap between slots: every block exact, nothing written
    before the first slot, behind the last or into a neighbour."""
    blocks, pb = packed
    caps = [len(w.want) for w in blocks]
    off = check_packed(blocks, pb, caps, [True] * len(blocks))
    for r in S.ROUTE_NAMES:
        assert {int(o) % 16 for o, w in zip(off, blocks) if w.route == r} == set(range(16)), r


def test_output_capacity_beyond_the_decoded_length(packed):
    """cap == D + 37: the slack behind each block stays as it was."""
    blocks, pb = packed
    check_packed(blocks, pb, [len(w.want) + 37 for w in blocks], [True] * len(blocks))


def test_output_capacity_one_byte_short(packed):
    """cap == D - 1 on every third block: PBL_OVERFLOW, out_len 0, its slot
    untouched; the others exact."""
    blocks, pb = packed
    fits = [i % 3 != 1 or not w.want for i, w in enumerate(blocks)]     # (an empty block has no byte to lose)
    assert {w.route for w, ok in zip(blocks, fits) if not ok} == set(S.ROUTE_NAMES)
    check_packed(blocks, pb, [len(w.want) - (0 if ok else 1) for w, ok in zip(blocks, fits)], fits)


def test_input_at_every_phase_from_the_first_byte_to_the_last():
    """The first block at device offset 0, the last block's trailer ending the
    tensor, and each route's blocks at each of the 16 input phases."""
    pool = {r: [w for w in S.sample_by_cell(S.wrapped_corpus(), 1) if w.route == r] for r in S.ROUTE_NAMES}
    blocks = [pool[r][p % len(pool[r])] for p in range(16) for r in S.ROUTE_NAMES]
    buf, off = bytearray(), []
    for i, w in enumerate(blocks):
        buf += bytes((i // 3 - len(buf)) % 16)     # phase i // 3 (the first block: 0, no pad)
        off.append(len(buf))
        buf += w.block + bytes([SNAPPY]) + bytes(4)
    assert off[0] == 0 and {(o % 16, w.route) for o, w in zip(off, blocks)} == {(p, r) for p in range(16) for r in S.ROUTE_NAMES}
    assert off[-1] + len(blocks[-1].block) + 5 == len(buf)
    pb = PhysBatch(torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(),
                   torch.from_numpy(np.asarray(off, np.int64)).cuda(),
                   torch.from_numpy(np.asarray([len(w.block) for w in blocks], np.int32)).cuda())
    assert pb.bytes.numel() == len(buf)
    check_packed(blocks, pb, [len(w.want) for w in blocks], [True] * len(blocks))
