"""Row blocks whose keys are longer than the general walk's 32 KiB LDS key
buffer (host only): a raw block builder with exact control of every entry's
shared length, and the block shapes the long-key tests decode.

C = 32768 is the buffer's capacity in key bytes: key byte p lives in LDS for
p < C and in the workspace's spill slot past it."""
import os

import numpy as np

C = 32768
KIND_SET, KIND_MERGE = 1, 2
OBSOLETE = 64  # InternalKeyKindSSTableInternalObsoleteBit in the trailer's kind byte
# internal key lengths: the last that fits in LDS, the first that does not, a
# 16-B window short of / at / past the seam, 40 KiB, 100 KiB
KEY_LENS = [32768, 32769, 32783, 32784, 32785, 40 * 1024, 100 * 1024]


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ikey(user: bytes, seq: int, kind: int = KIND_SET) -> bytes:
    return user + ((seq << 8) | kind).to_bytes(8, "little")


def user_bytes(n: int, seed: int) -> bytes:
    """n pseudo-random bytes (no two 16-B windows alike, so a misplaced window
    shows)."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def raw_row_block(entries, ri: int) -> bytes:
    """entries: [(key, value)] or [(key, value, shared)].  Entry i restarts a run
    when i % ri == 0 (shared 0); otherwise it shares the longest common prefix
    with the key before it, or exactly `shared` bytes when given (a shorter
    legal prefix, or an illegal one for the corrupt shapes)."""
    out, restarts, prev = bytearray(), [], b""
    for i, e in enumerate(entries):
        key, val = e[0], e[1]
        if i % ri == 0:
            restarts.append(len(out))
            sh = 0
        else:
            sh = len(os.path.commonprefix([prev, key]))
        if len(e) > 2 and e[2] is not None:
            sh = e[2]
        out += varint(sh) + varint(len(key) - min(sh, len(key))) + varint(len(val)) + key[sh:] + val
        prev = key
    if not restarts:
        restarts = [0]
    for r in restarts:
        out += r.to_bytes(4, "little")
    out += len(restarts).to_bytes(4, "little")
    return bytes(out)


def _val(i: int, n: int = 20) -> bytes:
    # a SET's value prefix byte first (block.ValuePrefix: 0x00 in place, 0x80 a
    # value-block handle), so that every shape is legal under PBL_ROW_VALUE_PREFIX
    return bytes([0x80 if i % 3 == 2 else 0x00]) + bytes([65 + i % 26]) * n


def shape_a(klen: int, seed: int = 1):
    """One user key under trailers that differ in one byte each: unshared 8,
    1 .. 7 and 0, the trailer partly or wholly out of the shared prefix."""
    u = user_bytes(klen - 8, seed)
    seqs = [0x11223344556677, 0x11223344556678, 0x11223344AA6678, 0x21223344AA6678, 0x21223344AA6678]
    return [(ikey(u, s, KIND_SET), _val(i)) for i, s in enumerate(seqs)]


def shape_b(klen: int, seed: int = 2):
    """Long, 100 B, long again sharing less than C with the first."""
    u = user_bytes(klen - 8, seed)
    short = u[:40] + user_bytes(52, seed + 100)
    again = u[:C - 5000] + user_bytes(klen - 8 - (C - 5000), seed + 200)
    return [(ikey(u, 9), _val(0)), (ikey(short, 8), _val(1)), (ikey(again, 7), _val(2)), (ikey(again, 6), _val(3))]


def shape_c(seed: int = 3):
    """Shared lengths ending at C-1, C, C+1 and C+17."""
    u = user_bytes(C + 3000, seed)
    out = [(ikey(u, 50), _val(0))]
    for i, sh in enumerate((C - 1, C, C + 1, C + 17)):
        k = u[:sh] + user_bytes(2000 + 7 * i, seed + 10 + i)
        if k[sh] == out[-1][0][sh]:
            k = k[:sh] + bytes([k[sh] ^ 1]) + k[sh + 1:]
        u = k
        out.append((ikey(k, 40 - i), _val(i + 1)))
    return out


def shape_d(seed: int = 4):
    """Keys growing by one byte each, across C."""
    u = user_bytes(C + 64, seed)
    return [(u[:C - 8 - 2 + i] + (5 << 8 | KIND_MERGE).to_bytes(8, "little"), _val(i, 3)) for i in range(6)]


def shape_e(klen: int, seed: int = 5):
    """A long key, then a shorter long key with unshared = 3: its trailer's
    bytes lie in the middle of the previous key, past C.  The second entry's
    shared length is given, so at restart interval 1 it is a restart point with
    a non-zero shared length, which no writer emits (the sequential decoders,
    Go's and the device's, read it all the same): the shape is a block a writer
    could have made only at restart intervals 2 and 16."""
    u = user_bytes(klen - 8, seed)
    first = ikey(u, 77, KIND_MERGE)
    cut = C + (klen - C) // 2
    second = first[:cut] + bytes([first[cut] ^ 0x10, 0x5A, 0xA5])
    return [(first, _val(0)), (second, _val(1), cut), (second[:-1] + b"\x01", _val(2))]


def shape_hide(klen: int, seed: int = 6):
    """HideObsoletePoints: an obsolete long key between two visible ones, the
    later sharing its spilled bytes; an obsolete entry last."""
    u = user_bytes(klen - 8, seed)
    mid = u[:C + 100] + user_bytes(klen - 8 - (C + 100), seed + 1)
    last = mid[:-30] + user_bytes(30, seed + 2)
    return [(ikey(u, 30), _val(0)), (ikey(mid, 29, KIND_SET | OBSOLETE), _val(1)), (ikey(last, 28), _val(2)),
            (ikey(last, 27, KIND_SET | OBSOLETE), _val(3))]


def long_key_blocks(ri: int):
    """[(name, block)]: every legal shape at restart interval `ri`.  The 100 KiB
    key sits in blocks of two or three entries (about 200 KiB at ri 1)."""
    out = []
    for kl in KEY_LENS:
        big = kl > 64 * 1024
        out.append((f"a klen={kl}", raw_row_block(shape_a(kl)[:3 if big else 5], ri)))
        if not big:
            out.append((f"e klen={kl}", raw_row_block(shape_e(kl + 40), ri)))
    out.append(("a user key ends within 8 bytes of C", raw_row_block(shape_a(C + 5), ri)))
    out.append(("b 40 KiB", raw_row_block(shape_b(40 * 1024), ri)))
    out.append(("b 100 KiB", raw_row_block(shape_b(100 * 1024)[:3], ri)))
    out.append(("c", raw_row_block(shape_c(), ri)))
    out.append(("d", raw_row_block(shape_d(), ri)))
    out.append(("e 100 KiB", raw_row_block(shape_e(100 * 1024)[:2], ri)))
    out.append(("hide 40 KiB", raw_row_block(shape_hide(40 * 1024), ri)))
    out.append(("hide 33 KiB", raw_row_block(shape_hide(C + 1024), ri)))
    return out


def corrupt_blocks(ri: int):
    """[(name, block)]: f. shared one more than the previous long key's length;
    g. a block cut inside a long key's unshared bytes (its restart table kept)."""
    ri = max(ri, 2)  # (the bad entry must not start a run)
    a = shape_a(40 * 1024)
    f = raw_row_block([a[0], (a[1][0] + b"xy", a[1][1], len(a[0][0]) + 1), a[2]], ri)
    b = shape_b(40 * 1024)
    whole = raw_row_block(b, 16)
    body = whole[:-8]
    cut = body[: len(body) - len(b[3][1]) - len(b[2][1]) - 3 - 1000]
    g = cut + whole[-8:]
    return [("f shared past the previous key", f), ("g cut inside a long key", g)]


def slot_loop_blocks(n: int, seed: int = 9):
    """n blocks of about 41 KiB, one 40 KiB key and three keys sharing it."""
    out = []
    for i in range(n):
        u = user_bytes(40 * 1024 - 8, seed + i)
        ents = [(ikey(u, 9), _val(i))] + [(ikey(u[:-4 * k] + bytes([i, k, 7, 9] * k), 9 - k), _val(k)) for k in (1, 2, 3)]
        out.append(raw_row_block(ents, 16))
    return out
