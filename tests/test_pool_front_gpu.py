"""The staging-pool row kernel's front (rowblk_pool.hip.h): the walk of the
restart runs, one run per lane with the run's first 16 entries parked in
registers, and the metadata pass that writes the slot from them.  The walk's
entries are straight-line code (a lane past its run's end or a failed lane
goes on with its results unused, the failure causes examined once after the
loop, the one-byte header form chosen by a ballot of the live lanes); the
metadata pass is 16 flat bodies.  Every fallback stays where it was: a run
past the 16 parked entries (the tail walk), more runs than lanes (the rolled
path), and the blocks the general walk takes.

Every case is decoded with PBL_KERNEL_POOL forced, twice into outputs filled
with 0xFF, at 16 shifts of the buffer (every block starts at all 16 values of
block_off & 15), and compared with the oracle bit-exact on every output array.
Blocks are at most 4 KiB (the few that must hold a 4 KiB key or a 16 KiB value
excepted) and a batch is a few hundred blocks."""
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, make_trailer
from test_rowblk_gpu import assert_same

pytestmark = pytest.mark.gpu
POOL = N.PBL_KERNEL_POOL
VP, NOV, RAW, HIDE = N.PBL_ROW_VALUE_PREFIX, N.PBL_ROW_NO_VALUER, N.PBL_ROW_RAW_KEYS, N.PBL_ROW_HIDE_OBSOLETE
SLOT_KV = 511  # entries a slot holds (Slot::kKv)
MAX_KL = 4095  # internal-key bytes on the fast path (kMaxKl)


# ---- blocks ---------------------------------------------------------------------
def kv(uk, seq=1, kind=1, val=b"", obs=False, vp=None, same=False, ms=None):
    """One entry: user key, sequence number, kind, value; `obs`: the obsolete
    bit; `vp`: a value prefix byte; `same`: setHasSameKeyPrefix; `ms`: the most
    key bytes it may share (default: the user key's length)."""
    return (uk, seq, kind, val, obs, vp, same, len(uk) if ms is None else ms)


def build(kvs, ri=16, limit=4096):
    w = Writer(ri)
    for uk, seq, kind, val, obs, vp, same, ms in kvs:
        w.add_with_optional_value_prefix(uk, make_trailer(seq, kind), obs, val, ms, vp is not None, vp or 0, same)
    b = w.finish()
    assert len(b) <= limit, len(b)
    return b


def build_raw(pairs, ri=16):
    w = Writer(ri)
    for k, v in pairs:
        w.add_raw(k, v)
    b = w.finish()
    assert len(b) <= 4096, len(b)
    return b


def varint(b, i):
    v, s = 0, 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 128:
            return v, i


def put_varint(v, pad=0):
    """The varint of v, padded with continuation bytes to `pad` bytes if longer."""
    out = []
    while v >= 128 or len(out) + 1 < pad:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out + [v])


def parse(blk):
    """(offset, shared, unshared, value length, header length) of every entry,
    the restart words, and the restart table's offset."""
    n = int.from_bytes(blk[-4:], "little")
    roff = len(blk) - 4 * (n + 1)
    rs = [int.from_bytes(blk[roff + 4 * i: roff + 4 * i + 4], "little") for i in range(n)]
    ents, p = [], 0
    while p < roff:
        sh, a = varint(blk, p)
        un, b = varint(blk, a)
        vl, c = varint(blk, b)
        ents.append((p, sh, un, vl, c - p))
        p = c + un + vl
    assert p == roff
    return ents, rs, roff


def hdr_lens(blk):
    """Per entry: the byte lengths of its three header varints."""
    out = []
    for p, sh, un, vl, h in parse(blk)[0]:
        out.append(tuple(len(put_varint(x)) for x in (sh, un, vl)))
    return out


def seq_block(n, ri, ukl=8, vl=8, seed=0, **kw):
    """n entries with keys in order, restart interval ri."""
    rng = random.Random(seed)
    return build([kv(b"%0*d" % (ukl, k), 100 + k, 1 if k % 3 else 2, rng.randbytes(vl), **kw) for k in range(n)], ri)


# ---- decode ---------------------------------------------------------------------
def pack_at(blocks, shift):
    """The blocks back to back, the first at byte `shift`."""
    offs, pos = [], shift
    for b in blocks:
        offs.append(pos)
        pos += len(b)
    buf = np.zeros(pos + 16, np.uint8)
    for o, b in zip(offs, blocks):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return buf, np.array(offs, np.uint64), np.array([len(b) for b in blocks], np.uint32)


def run(blocks, flags=0, ctx="", shifts=range(16)):
    """Decode at every shift, twice into dirty outputs; the oracle runs once
    (its result does not depend on where the blocks lie)."""
    import torch
    from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode_into
    o, g = None, None
    for sh in shifts:
        buf, off, lens = pack_at(blocks, sh)
        if o is None:
            o = oracle.decode_batch(buf, off, lens, 0, None, flags) if flags & HIDE else \
                oracle.rowblk_decode_batch(buf, off, lens, flags)
            cap = Capacity(kv=o["n_kv"], key=o["key_bytes_total"], val=o["val_bytes_total"], rst=o["n_restarts"])
        b = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, flags | POOL)
        out = DecodedBatch.allocate(b.n_blocks, cap, "cuda")
        for rnd in range(2):
            for t in (out.workspace, out.totals, out.blk_status, out.blk_kv_base, out.blk_key_base, out.blk_val_base,
                      out.blk_rst_base):
                t.view(torch.uint8).fill_(0xFF)
            decode_into(b, out)
            torch.cuda.synchronize()
            g = out.to_host()
            assert not g["status_mask"] & (1 << N.PBL_TIMEOUT), f"{ctx} shift {sh} round {rnd}: PBL_TIMEOUT"
            assert_same(g, o, f"{ctx} shift {sh} round {rnd}")
    return g, o


def fill(blocks, n=256):
    """The blocks repeated to a batch of about n, in a fixed shuffled order."""
    out = blocks * max(1, n // len(blocks))
    random.Random(len(blocks)).shuffle(out)
    return out


# ---- the shapes -----------------------------------------------------------------
def run_length_blocks():
    out = [build([]), seq_block(1, 16)]  # an empty block; a block of one entry
    for ri in (1, 2, 15, 16, 17, 31, 33):  # 17 and up: `over` and the tail walk
        for n in (ri, ri + 1, 2 * ri, 2 * ri + 1, 3 * ri - 1):  # (ri + 1, 2 ri + 1: a last run of one entry)
            out.append(seq_block(n, ri, seed=ri + n))
    return out


def run_count_blocks():
    """Restart interval 1: a run per entry.  64 runs: one per lane; 65, 128: the rolled path."""
    return [seq_block(n, 1, ukl=4, vl=4, seed=n) for n in (1, 2, 63, 64, 65, 128)]


def past_slot_blocks():
    """More entries than a slot holds: the general walk."""
    out = []
    for n in (SLOT_KV, SLOT_KV + 1, SLOT_KV + 9):
        # (3-byte keys after the first: those KVs are PBL_KV_INVALID_KEY unless raw)
        b = build_raw([(b"00000000", b"")] + [(b"%03d" % k, b"") for k in range(1, n)], 16)
        assert len(parse(b)[0]) == n
        out.append(b)
    return out


def header_blocks():
    rng = random.Random(3)
    long_a, long_b = b"a" * 150, b"a" * 150 + b"b" * 140
    one = seq_block(20, 16, seed=1)
    sh2 = build([kv(long_a + b"%02d" % k, 9, 1, b"v") for k in range(6)], 16)         # shared >= 128 alone
    un2 = build([kv(b"%c" % (65 + k) + long_a, 9, 1, b"v") for k in range(6)], 1)     # unshared >= 128 alone
    vl2 = build([kv(b"%08d" % k, 9, 1, rng.randbytes(128 + 40 * k)) for k in range(6)], 16)  # value >= 128 alone
    all3 = build([kv(long_a, 9, 1, b"v"), kv(long_b, 8, 1, rng.randbytes(200)),
                  kv(long_a + b"c" * 140, 7, 1, rng.randbytes(300))], 16)
    # lanes that mix one- and two-byte headers at the same unrolled position:
    # restart interval 2, the runs' values alternately short and long
    mixed = build([kv(b"%08d" % k, 9, 1, rng.randbytes(130 if (k // 2) % 2 else 5)) for k in range(24)], 2)
    H = [hdr_lens(b) for b in (one, sh2, un2, vl2, all3, mixed)]
    assert set(H[0]) == {(1, 1, 1)}
    assert (2, 1, 1) in H[1] and (1, 2, 1) in H[2] and (1, 1, 2) in H[3] and (2, 2, 2) in H[4]
    assert H[5][1] == (1, 1, 1) and H[5][3] == (1, 1, 2)
    return [one, sh2, un2, vl2, all3, mixed]


def three_byte_block():
    """A 16 KiB value (a 3-byte value length) among short entries: one block of about 17 KiB."""
    rng = random.Random(4)
    b = build([kv(b"%08d" % k, 9, 1, rng.randbytes(16400 if k == 5 else 9)) for k in range(20)], 16, limit=20000)
    assert (1, 1, 3) in hdr_lens(b)
    return b


def four_byte_block():
    """The last entry's value length re-encoded in four bytes (a padded varint;
    one run, so no restart offset moves): the general walk."""
    b = seq_block(12, 16, seed=5)
    ents, rs, roff = parse(b)
    p, sh, un, vl, h = ents[-1]
    assert rs == [0] and max(sh, un, vl) < 128 and h == 3
    nb = b[:p + 2] + put_varint(vl, 4) + b[p + 3:]
    assert parse(nb)[0][-1] == (p, sh, un, vl, 6)
    return nb


def key_blocks():
    rng = random.Random(6)
    out = []
    # keys shorter than 8 B (PBL_KV_INVALID_KEY), not first in the block, and of exactly 8
    out.append(build([kv(b"", 5, 1, b"v0")] + [kv(b"%d" % k, 5, 1, b"v") for k in range(1, 9)], 4))
    w = Writer(4)
    w.add(b"first", make_trailer(3, 1), b"x")
    for k in range(12):
        w.add_raw(b"k%d" % k if k % 3 else b"kkkkkk%02d" % k, b"v%d" % k)  # 2-3 B and 8 B keys
    out.append(w.finish())
    # every key's prefix parent is its predecessor
    out.append(build([kv(b"run%04d" % (k // 16) + b"x" * (k % 16), 9, 1, rng.randbytes(7)) for k in range(50)], 16))
    # shared lengths rise and fall: the parent search walks several hops
    stairs = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdef", b"abd", b"abda", b"abdab", b"abdabc", b"abdabcd",
              b"abe", b"ac", b"acaaaa", b"acaaab", b"acab", b"b"]
    out.append(build([kv(u + b"\xff", 9, 1, rng.randbytes(5)) for u in stairs], 32))
    out.append(build([kv(u + b"\xff", 9, 1, rng.randbytes(5)) for u in stairs[:16]], 16))
    sh = [e[1] for e in parse(out[-1])[0]]
    assert sh[:7] == [0, 1, 2, 3, 4, 5, 2] and sh[11:13] == [2, 1], sh
    # the restart word's same-prefix bit
    b = build([kv(b"pfx%05d" % (k // 8), 100 - k % 8, 1, b"v", same=k % 8 != 0) for k in range(40)], 4)
    assert any(r >> 31 for r in parse(b)[1]) and not all(r >> 31 for r in parse(b)[1])
    out.append(b)
    return out


def long_key_blocks():
    """Internal keys of 4095 B (the fast path's longest) and 4096 B (the general
    walk); these two blocks are past 4 KiB because a key of theirs is."""
    u = b"k" * (MAX_KL - 8 - 2)
    ok = build([kv(u + b"aa", 9, 1, b"v"), kv(u + b"ab", 8, 1, b"w"), kv(u + b"b", 7, 1, b"x")], 16, limit=4400)
    over = build([kv(u + b"aa", 9, 1, b"v"), kv(u + b"aab", 8, 1, b"w"), kv(u + b"b", 7, 1, b"x")], 16, limit=4400)
    kl = lambda b: [e[1] + e[2] for e in parse(b)[0]]
    assert kl(ok) == [MAX_KL, MAX_KL, MAX_KL - 1] and kl(over) == [MAX_KL, MAX_KL + 1, MAX_KL - 1]
    return [ok, over]


def value_prefix_blocks():
    """SET values with each prefix class next to other kinds without a prefix."""
    rng = random.Random(7)
    out = []
    for ri, n in ((16, 40), (5, 33), (17, 40), (1, 70)):
        kvs = []
        for k in range(n):
            kind = 1 if k % 4 else (0, 2)[k // 4 % 2]
            kvs.append(kv(b"%08d" % k, 100 + k, kind, rng.randbytes((0, 1, 9, 30)[k % 4] if kind == 1 else k % 3),
                          vp=(0x00, 0x80, 0xC0)[k % 3] if kind == 1 else None))
        out.append(build(kvs, ri))
    return out


def empty_set_block():
    """A SET whose value lacks even the prefix byte: PBL_CORRUPT_BOUNDS when values carry prefixes."""
    return build([kv(b"%08d" % k, 9, 1, b"" if k == 6 else b"val", vp=None if k == 6 else 0) for k in range(20)], 16)


def hide_blocks():
    rng = random.Random(8)
    # the kind byte among the unshared bytes
    own = [seq_block(n, ri, seed=n, obs=False) for n, ri in ((20, 16), (40, 17))]
    own += [build([kv(b"%08d" % k, 100 + k, 1 if k % 3 else 2, rng.randbytes(6), obs=k % every == every - 1)
                   for k in range(n)], ri) for n, ri, every in ((50, 16, 2), (33, 4, 5), (40, 17, 3), (64, 1, 2))]
    # the kind byte inside the shared prefix, key lengths equal: the same user
    # key and kind, sequence numbers that differ above their low byte
    eq = build([kv(b"samekey%d" % (k // 8), (9 - k % 8) << 8 | 5, 1, b"v%d" % k, obs=(k // 8) % 2 == 1, ms=64)
                for k in range(32)], 16)
    e = parse(eq)[0]
    assert all(sh + un == 16 for _, sh, un, _, _ in e) and e[1][1] >= 10 and e[1][2] < 8
    # ... and key lengths unequal (a user key that ends like the next key's
    # trailer begins): the general walk
    t = make_trailer(5, 1).to_bytes(8, "little")
    ne = build([kv(b"kkkk" + t[:2], 7, 1, b"a"), kv(b"kkkk", 5, 1, b"b", ms=64), kv(b"kkkl", 5, 1, b"c")], 16)
    e = parse(ne)[0]
    assert e[1][1] == 6 and e[0][1] + e[0][2] == 14 and e[1][1] + e[1][2] == 12
    return own, eq, ne


def corrupt_blocks():
    """Writer output with one byte patched (every patched varint stays one
    byte).  A forward iteration reads no restart word and takes any shared
    length up to the previous key's, so two of these decode without an error,
    off the lane-per-run walk; the others are PBL_CORRUPT_BOUNDS."""
    out = {}
    base = seq_block(40, 8, seed=9)
    ents, rs, roff = parse(base)
    assert all(max(e[1:4]) < 128 for e in ents)
    b = bytearray(base)
    b[rs[2]] = 1  # shared != 0 at the third run's restart
    out["shared at a restart"] = bytes(b)
    b = bytearray(base)
    p = ents[15][0]  # the last entry of the second run: its value runs into the third
    b[p + 2] += 30
    out["entry past its run"] = bytes(b)
    b = bytearray(base)
    b[ents[23][0] + 2] = 127  # the last run's entries end past the restart table
    out["entry past its run, late"] = bytes(b)
    b = bytearray(base)
    b[ents[10][0]] = 100  # shared > the previous key's 16 bytes
    out["shared past the previous key"] = bytes(b)
    b = bytearray(base)
    b[roff + 4: roff + 8], b[roff + 8: roff + 12] = b[roff + 8: roff + 12], b[roff + 4: roff + 8]
    out["restarts out of order"] = bytes(b)
    return out


# ---- the tests ------------------------------------------------------------------
def test_run_lengths_around_the_parked_sixteen():
    g, o = run(fill(run_length_blocks()), 0, "run lengths")
    assert g["status_mask"] == 0 and g["n_kv"] > 0


def test_run_counts_around_a_wave():
    blocks = run_count_blocks()
    g, o = run(fill(blocks, 192), 0, "run counts")
    assert g["status_mask"] == 0
    for b in blocks:
        run([b], 0, f"{len(parse(b)[1])} runs alone", shifts=(0, 7))


@pytest.mark.parametrize("flags", [0, RAW, HIDE])
def test_entries_past_the_slot(flags):
    blocks = past_slot_blocks()
    g, o = run(fill(blocks + [seq_block(30, 16)], 64), flags, f"past the slot, flags {flags:#x}")
    assert g["status_mask"] == 0


def test_header_forms():
    g, o = run(fill(header_blocks() + [four_byte_block()]), 0, "header forms")
    assert g["status_mask"] == 0
    run([four_byte_block()], 0, "four-byte varint alone", shifts=(0, 5))


def test_three_byte_value_length():
    big = three_byte_block()
    g, o = run([seq_block(20, 16), big, seq_block(33, 16), big], 0, "16 KiB value")
    assert g["status_mask"] == 0


def test_keys():
    g, o = run(fill(key_blocks()), 0, "keys")
    assert g["status_mask"] == 0
    assert (o["kv_flags"] & N.PBL_KV_INVALID_KEY).any() and (o["kv_flags"] & N.PBL_KV_RESTART_SAMEPFX).any()
    run(fill(key_blocks(), 64), RAW, "keys, raw")


def test_longest_fast_key():
    ok, over = long_key_blocks()
    g, o = run([ok, over, seq_block(20, 16), ok, over, over, ok] * 6, 0, "4095 and 4096 B keys")
    assert g["status_mask"] == 0


@pytest.mark.parametrize("flags", [VP, VP | NOV, VP | HIDE])
def test_value_prefix(flags):
    blocks = value_prefix_blocks()
    g, o = run(fill(blocks), flags, f"value prefix, flags {flags:#x}")
    assert g["status_mask"] == 0
    handles = N.PBL_KV_VALBLK_HANDLE | N.PBL_KV_BLOB_HANDLE
    assert bool((o["kv_flags"] & handles).any()) == (not flags & NOV)
    g, o = run(fill(blocks + [empty_set_block()], 64), flags, f"an empty SET value, flags {flags:#x}")
    assert g["status_mask"] == 1 << N.PBL_CORRUPT_BOUNDS and g["n_bad_blocks"] == 64 // 5


def test_raw_keys():
    g, o = run(fill(run_length_blocks() + key_blocks() + header_blocks()), RAW, "raw keys")
    assert g["status_mask"] == 0


def test_hide_obsolete():
    own, eq, ne = hide_blocks()
    g, o = run(fill(own), HIDE, "hide, kind byte unshared")
    assert g["status_mask"] == 0 and 0 < g["n_kv"]
    g, o = run(fill(own + [eq], 64), HIDE, "hide, kind byte shared, equal lengths")
    assert g["status_mask"] == 0
    g, o = run(fill(own + [eq, ne], 64), HIDE, "hide, kind byte shared, unequal lengths")
    assert g["status_mask"] == 0
    for b in (eq, ne):
        run([b], HIDE, "alone", shifts=(0, 9))
        run([b], 0, "alone, not hiding", shifts=(0, 9))


@pytest.mark.parametrize("flags", [0, HIDE, VP])
def test_corrupt_blocks(flags):
    bad = corrupt_blocks()
    good = seq_block(40, 8, seed=9)
    for name, b in bad.items():
        g, o = run([good, b, good], flags, name, shifts=(0, 3))
        assert o["blk_status"][0] == o["blk_status"][2] == N.PBL_OK, name
        assert (o["blk_status"][1] == N.PBL_OK) == (name in ("shared at a restart", "restarts out of order")), name
    g, o = run(fill(list(bad.values()) + [good] * 3, 96), flags, f"corrupt blocks, flags {flags:#x}")
    assert g["n_bad_blocks"] == 12 * 3 and g["status_mask"] == 1 << N.PBL_CORRUPT_BOUNDS


@pytest.mark.parametrize("flags", [0, HIDE, VP])
def test_mixed_batch(flags):
    """Fast, `over`, rolled and general-walk blocks alternating on a CU's waves."""
    own, eq, ne = hide_blocks()
    blocks = run_length_blocks() + run_count_blocks() + past_slot_blocks()[:2] + header_blocks() + \
        [four_byte_block()] + key_blocks() + value_prefix_blocks() + own + [eq, ne] + list(corrupt_blocks().values())
    if flags & VP:
        blocks.append(empty_set_block())
    g, o = run(fill(blocks, 300), flags, f"mixed batch, flags {flags:#x}")
    assert g["n_bad_blocks"] > 0 and g["n_kv"] > 0
