"""The staging-pool row kernel's emit steps (rowblk_pool.hip.h): a step of 64
KVs copies its values either as the fast straight-line step (every value empty
or 16..128 B, descriptors read once and permuted to the 8-lane groups) or as
the general step, the class decided at the step's loads and used one iteration
later at its stores; the step's accesses address a uniform base plus an
unsigned 32-bit lane offset, the fast value loads from the block's pointer
aligned down to 16 B, and a key whose 16-B window touches the block's first or
last granule leaves the fast key form.

Every case is decoded with PBL_KERNEL_POOL forced and compared with the oracle,
bit-exact on every output array.  Blocks are at most 4 KiB and a batch is a few
hundred blocks."""
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, make_trailer
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
POOL = N.PBL_KERNEL_POOL
STEP = 64

# the value lengths around every threshold of the value copy: the byte loop
# (< 16), one chunk per lane (16..128), further chunks (129..1024), the
# whole-wave copy (> 1024)
SHORT = [0, 1, 15, 16, 17, 31, 32, 100, 112, 127, 128, 129, 130]
LONG = [1023, 1024, 1025]
FAST = [0, 16, 17, 31, 32, 100, 112, 127, 128]
BREAKERS = [1, 15, 129, 130, 1023, 1024, 1025]


def user_key(k, ukl):
    return b"%0*d" % (ukl, k) if ukl else b""


def block(vls, ukl=8, ri=16, obsolete=0, vp=False, deep=False, seed=0):
    """One row block of len(vls) KVs with those value lengths.  `obsolete` n:
    every n-th KV carries the obsolete bit; `vp`: SET values with a value
    prefix byte; `deep`: the keys of a run grow by one byte each, so a key's
    prefix chain runs through every earlier key of its run."""
    rng = random.Random(seed)
    w = Writer(ri)
    for k, vl in enumerate(vls):
        uk = b"run%04d" % (k // ri) + b"x" * (k % ri) if deep else user_key(k, ukl)
        kind = 1 if vp or k % 3 else 2
        val = rng.randbytes(vl)
        obs = bool(obsolete) and k % obsolete == obsolete - 1
        w.add_with_optional_value_prefix(uk, make_trailer(100 + k, kind), obs, val, len(uk), vp and kind == 1,
                                         (0x00, 0x80, 0xC0)[k % 3], False)
    b = w.finish()
    assert len(b) <= 4096, len(b)
    return b


def check(blocks, flags=0, ctx="", align=1):
    from pebble_amd.batch import BlockBatch, decode
    buf, off, lens = pack(blocks, align)
    hide = flags & N.PBL_ROW_HIDE_OBSOLETE
    o = oracle.decode_batch(buf, off, lens, 0, None, flags) if hide else oracle.rowblk_decode_batch(buf, off, lens, flags)
    g = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags | POOL)).to_host()
    assert_same(g, o, ctx)
    return g, o


def mixed_lengths(seed):
    """Every short length and one long one in one block, shuffled."""
    rng = random.Random(seed)
    vls = SHORT + [LONG[seed % 3]] + [rng.choice(FAST[:5]) for _ in range(52)]  # two steps, under 4 KiB
    rng.shuffle(vls)
    return vls


def one_breaker(n, pos, brk, fill=16):
    vls = [fill] * n
    vls[pos] = brk
    return vls


def alternating(first_general):
    """Four steps whose classes alternate: a lone breaker in every other step."""
    vls = []
    for s in range(4):
        step = [(0, 0, 16, 0)[k % 4] for k in range(STEP)]
        if (s % 2 == 0) == first_general:
            step[(7 * s + 5) % STEP] = (15, 129, 1, 130)[s]
        vls += step
    return vls[:193]  # (the fourth step partial, its breaker inside; under 4 KiB)


@pytest.fixture(scope="module")
def step_blocks():
    """The blocks where the fast / general split can go wrong, shared by the tests."""
    out = []
    for n in (0, 1, 63, 64, 65, 127, 128, 129):  # the last partial step; the step that only writes the nkv-th offsets
        out.append(block([16] * n, seed=n))
        out.append(block([(0, 100, 17, 32)[k % 4] for k in range(n)] if n < 100 else [(0, 16)[k % 2] for k in range(n)], seed=n + 1))
        out.append(block([15] * n, seed=n + 2))  # every step general
    for s in range(6):
        out.append(block(mixed_lengths(s), seed=40 + s))
    n = 80
    for pos in (0, 63, 64, n - 1):  # exactly one KV of a step off the fast class
        for i, brk in enumerate(BREAKERS):
            out.append(block(one_breaker(n, pos, brk, (16, 0, 17)[i % 3]), seed=100 + pos + i))
    out.append(block(alternating(True), seed=7))
    out.append(block(alternating(False), seed=8))
    return out


def test_kv_counts_lengths_and_classes(step_blocks):
    g, o = check(step_blocks * 3, 0, "steps")
    assert g["status_mask"] == 0 and g["n_kv"] == o["n_kv"] > 0
    for i, b in enumerate(step_blocks):  # and each block first in a batch of its own kind
        check([b], 0, f"block {i} alone")


def test_all_sixteen_phases_back_to_back(step_blocks):
    """Blocks of varying length packed with no padding: block_off & 15 takes
    every phase, the first block of the buffer and the last included."""
    rng = random.Random(9)
    blocks = [step_blocks[rng.randrange(len(step_blocks))] for _ in range(300)]
    # the buffer's first and last block run through every phase in turn
    for ph in range(16):
        lead = block([16] * 3 + [0] * ph, ukl=0, seed=ph)
        tail = block([128, 16, 100], seed=ph)
        order = [lead] + blocks[ph::16] + [tail]
        check(order, 0, f"phase run {ph}")
    buf, off, lens = pack(blocks, 1)
    assert set(int(x) & 15 for x in off) == set(range(16))
    tails = set(int(o + n) & 15 for o, n in zip(off, lens))
    assert tails == set(range(16))
    check(blocks, 0, "back to back")


@pytest.mark.parametrize("ukl", [0, 8, 16, 17])
def test_key_lengths_next_to_fast_steps(ukl):
    blocks = [block(mixed_lengths(s), ukl=ukl, seed=s) for s in range(4)]
    blocks += [block([(16, 100, 0, 0, 32, 0)[k % 6] for k in range(n)], ukl=ukl, seed=n) for n in (1, 64, 65, 100)]
    check(blocks * 8, 0, f"user keys of {ukl} B")


def test_deep_prefix_chain_next_to_fast_steps():
    blocks = [block(mixed_lengths(s), deep=True, seed=s) for s in range(4)]
    blocks += [block([(16, 128, 0, 0, 17, 0)[k % 6] for k in range(n)], deep=True, ri=ri, seed=n) for n, ri in ((64, 16), (65, 8), (100, 32))]
    check(blocks * 8, 0, "deep chains")


@pytest.mark.parametrize("every", [2, 5])
def test_hide_obsolete(every):
    blocks = [block(mixed_lengths(s), obsolete=every, seed=s) for s in range(4)]
    blocks += [block([16] * n, obsolete=every, seed=n) for n in (1, 2, 64, 65, 128, 129, 130)]
    blocks += [block(one_breaker(100, pos, brk), obsolete=every, seed=pos) for pos, brk in ((0, 15), (64, 129), (99, 1))]
    blocks += [block(alternating(True), obsolete=every, seed=3)]
    g, o = check(blocks * 6, N.PBL_ROW_HIDE_OBSOLETE, f"hide, every {every}th obsolete")
    assert 0 < g["n_kv"] < sum(6 * n for n in (1, 2, 64, 65, 128, 129, 130)) + 6 * 8 * 130


@pytest.mark.parametrize("flags", [N.PBL_ROW_VALUE_PREFIX, N.PBL_ROW_RAW_KEYS,
                                   N.PBL_ROW_VALUE_PREFIX | N.PBL_ROW_HIDE_OBSOLETE])
def test_value_prefix_and_raw_keys(flags, step_blocks):
    vp = bool(flags & N.PBL_ROW_VALUE_PREFIX)
    # (a stripped prefix byte moves every length down by one: 16 -> 15, 129 -> 128, 17 -> 16)
    blocks = [block(mixed_lengths(s), vp=vp, obsolete=3 if flags & N.PBL_ROW_HIDE_OBSOLETE else 0, seed=s) for s in range(6)]
    blocks += [block([(17, 16, 0, 1, 129, 0, 0, 0)[k % 8] for k in range(n)], vp=vp, seed=n) for n in (1, 64, 65, 90)]
    check(blocks * 6, flags, f"flags {flags:#x}")
    if not vp:
        check(step_blocks, flags, f"step blocks, flags {flags:#x}")


def test_exact_and_short_capacity(step_blocks):
    """Outputs sized exactly by a first decode: every store in bounds (guard
    bytes behind the value and key bytes stay untouched).  One value byte
    short: the blocks that no longer fit report PBL_OVERFLOW, the rest are
    written, sizes stay exact."""
    import torch
    from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode_into
    blocks = step_blocks * 2
    nb = len(blocks)
    buf, off, lens = pack(blocks, 1)
    g, o = check(blocks, 0, "first decode")
    full = Capacity(kv=g["n_kv"], key=g["key_bytes_total"], val=g["val_bytes_total"], rst=g["n_restarts"])
    batch = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, POOL)

    def run(cap):
        out = DecodedBatch.allocate(nb, cap, "cuda")
        guards = {}
        for name, n in (("val_bytes", cap.val), ("key_bytes", cap.key)):
            big = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
            setattr(out, name, big[:max(n, 1)])
            guards[name] = (big, n)
        decode_into(batch, out)
        torch.cuda.synchronize()
        for name, (big, n) in guards.items():
            assert bool((big[max(n, 1):] == 0xA5).all()), f"{name}: a store past the capacity"
        return out

    out = run(full)
    assert_same(out.to_host(), o, "exact capacity")
    assert out.read_totals().status_mask == 0

    vb = o["blk_val_base"]
    short = Capacity(kv=full.kv, key=full.key, val=full.val - 1, rst=full.rst)
    out = run(short)
    t = out.read_totals()
    want = np.where(vb[1:] > short.val, N.PBL_OVERFLOW, N.PBL_OK).astype(np.uint32)
    first = int(np.argmax(want == N.PBL_OVERFLOW))
    assert want[first] == N.PBL_OVERFLOW and first > 0
    assert np.array_equal(out.blk_status.cpu().numpy().view(np.uint32), want)
    assert (t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts) == \
        (o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"])
    assert t.status_mask == 1 << N.PBL_OVERFLOW and t.n_bad_blocks == int((want == N.PBL_OVERFLOW).sum())
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base"):
        assert np.array_equal(getattr(out, k).cpu().numpy().view(np.uint64), o[k]), k
    n, nk, nv = int(o["blk_kv_base"][first]), int(o["blk_key_base"][first]), int(vb[first])
    assert np.array_equal(out.trailer[:n].cpu().numpy().view(np.uint64), o["trailer"][:n])
    assert np.array_equal(out.val_off[:n + first].cpu().numpy().view(np.uint32), o["val_off"][:n + first])
    assert np.array_equal(out.key_bytes[:nk].cpu().numpy(), o["key_bytes"][:nk])
    assert np.array_equal(out.val_bytes[:nv].cpu().numpy(), o["val_bytes"][:nv])
