"""Helpers of the batched-seek tests (tests/test_seek.py, tests/test_seek_gpu.py):
restatements of the comparers, random key and block builders (as
tests/test_blockiter.py builds them), and the expected result of a batched
seek from the one-key host iterator (pebble_amd.blockiter.DataIter)."""
import functools
import struct

import numpy as np

from pebble_amd import _native as N
from pebble_amd.blockiter import DataIter, key_compare, key_split
from pebble_amd.rowblk import Writer, make_trailer

NONE = N.PBL_SEEK_NONE


def tk_compare(a: bytes, b: bytes) -> int:  # testkeys.compare (internal/testkeys/testkeys.go:136-171)
    def split(k):
        i = k.rfind(b"@")
        return i if i >= 0 else len(k)

    ai, bi = split(a), split(b)
    if a[:ai] != b[:bi]:
        return -1 if a[:ai] < b[:bi] else 1
    sa, sb = a[ai:].removesuffix(b"_synthetic"), b[bi:].removesuffix(b"_synthetic")
    if not sa or not sb:
        return (len(sa) > len(sb)) - (len(sa) < len(sb))
    x, y = int(sa[1:]), int(sb[1:])
    return (y > x) - (y < x)


def crdb_compare(a: bytes, b: bytes) -> int:  # cockroachkvs.Compare (cockroachkvs.go:313-339)
    if not a or not b:
        return (len(a) > len(b)) - (len(a) < len(b))
    asl, bsl = a[-1], b[-1]
    pa, pb = a[:len(a) - asl], b[:len(b) - bsl]
    if pa != pb:
        return -1 if pa < pb else 1
    if asl == 0 or bsl == 0:
        return (asl > bsl) - (asl < bsl)

    def norm(s):
        v = s[:-1]
        if len(v) == 13:
            v = v[:12]
        if len(v) == 12 and v[8:] == b"\0\0\0\0":
            v = v[:8]
        return v

    x, y = norm(a[len(a) - asl:]), norm(b[len(b) - bsl:])
    return (y > x) - (y < x)


CMP = {N.PBL_CMP_DEFAULT: lambda a, b: (a > b) - (a < b), N.PBL_CMP_TESTKEYS: tk_compare,
       N.PBL_CMP_CRDB: crdb_compare}


def crdb_key(rng, roach):
    r = rng.random()
    if r < 0.2:
        return roach + b"\x00"  # no version
    if r < 0.6:
        return roach + b"\x00" + struct.pack(">Q", rng.choice([1, 5, 1 << 40, rng.getrandbits(63)])) + b"\x09"
    if r < 0.8:
        lg = rng.choice([0, 1, 7])
        return roach + b"\x00" + struct.pack(">QI", rng.choice([1, 5, 1 << 40]), lg) + b"\x0d"
    if r < 0.9:
        return roach + b"\x00" + struct.pack(">QI", rng.choice([1, 5]), 0) + b"\x01" + b"\x0e"
    return roach + b"\x00" + bytes(rng.getrandbits(8) for _ in range(17)) + b"\x12"  # lock-table version


def keyfn(rng, comparer, roaches=(b"k1", b"k2", b"k3")):
    if comparer == N.PBL_CMP_TESTKEYS:
        return lambda: rng.choice([b"a", b"b", b"bb", b"c"]) + b"@" + str(rng.randrange(1, 30)).encode()
    if comparer == N.PBL_CMP_CRDB:
        return lambda: crdb_key(rng, rng.choice(roaches))
    return lambda: bytes(rng.choice(b"abc") for _ in range(rng.randrange(1, 5)))


class Seq:
    """Sequence numbers unique over a whole test input: (user key, trailer) names a KV."""

    def __init__(self):
        self.n = 0

    def next(self, kind=1):
        self.n += 1
        return make_trailer(self.n, kind)


def block_of(rng, seq, keys, obsolete=0.2, restart=None):
    """A row block of sorted user keys, one to two KVs each (as
    test_blockiter._random_block), each with its own sequence number."""
    w = Writer(restart or rng.choice([1, 2, 4, 16]))
    for k in keys:
        for _ in range(rng.choice([1, 1, 2])):
            v = bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 20])))
            w.add_with_optional_value_prefix(k, seq.next(rng.choice([1, 1, 0])), rng.random() < obsolete, v, len(k),
                                             False, 0, False)
    return w.finish()


def sorted_keys(comparer, keys):
    return sorted(set(keys), key=functools.cmp_to_key(CMP[comparer]))


def block_keys(h, b):
    kv0, kv1 = int(h["blk_kv_base"][b]), int(h["blk_kv_base"][b + 1])
    ko = h["key_off"][kv0 + b: kv1 + b + 1].astype(np.int64)
    kb = int(h["blk_key_base"][b])
    return [h["key_bytes"][kb + ko[j]: kb + ko[j + 1]].tobytes() for j in range(kv1 - kv0)]


def trailer_index(h):
    """(user key, trailer) -> global KV index: the internal key names the KV."""
    idx = {}
    for b in range(len(h["blk_status"])):
        kv0 = int(h["blk_kv_base"][b])
        for j, k in enumerate(block_keys(h, b) if int(h["blk_status"][b]) == 0 else []):
            idx[(k, int(h["trailer"][kv0 + j]))] = kv0 + j
    n_ok = sum(int(h["blk_kv_base"][b + 1] - h["blk_kv_base"][b]) for b in range(len(h["blk_status"]))
               if int(h["blk_status"][b]) == 0)
    assert len(idx) == n_ok, "internal keys must be unique in a seek test input"
    return idx


def _flags(comparer, op, key, kv):
    f = 0
    if op == "ge" and key_compare(comparer, kv.user_key, key) == 0:
        f |= N.PBL_SEEK_EXACT
    if kv.user_key[:key_split(comparer, kv.user_key)] == key[:key_split(comparer, key)]:
        f |= N.PBL_SEEK_SAME_PREFIX
    return f


def expected(h, keys, op, comparer, blocks=None, hide=False, tidx=None):
    """(kv, block, flags) lists a batched seek must give, from DataIter.SeekGE /
    SeekLT, one key at a time.  Table mode (blocks None): the PBL_OK blocks in
    batch order (SeekGE: the first that lands; SeekLT: the last)."""
    tidx = tidx if tidx is not None else trailer_index(h)
    nb = len(h["blk_status"])
    its = {}

    def it(b):
        if b not in its:
            its[b] = DataIter(h, b, comparer, hide)
        return its[b]

    kvs, blks, fls = [], [], []
    for i, key in enumerate(keys):
        res = (NONE, 0, 0)
        if blocks is not None:
            b = int(blocks[i])
            if b >= nb or int(h["blk_status"][b]) != 0:
                res = (NONE, 0, N.PBL_SEEK_BAD_BLOCK)
            else:
                kv = it(b).SeekGE(key) if op == "ge" else it(b).SeekLT(key)
                if kv is not None:
                    res = (tidx[(kv.user_key, kv.trailer)], b, _flags(comparer, op, key, kv))
        else:
            order = range(nb) if op == "ge" else range(nb - 1, -1, -1)
            for b in order:
                if int(h["blk_status"][b]) != 0:
                    continue
                kv = it(b).SeekGE(key) if op == "ge" else it(b).SeekLT(key)
                if kv is not None:
                    res = (tidx[(kv.user_key, kv.trailer)], b, _flags(comparer, op, key, kv))
                    break
        kvs.append(res[0])
        blks.append(res[1])
        fls.append(res[2])
    return kvs, blks, fls


def assert_seek(got, exp, ctx=""):
    """got: (kv, block, flags) arrays; exp: the lists of expected()."""
    kv, blk, fl = (np.asarray(x) for x in got)
    ekv = np.array(exp[0], np.uint64)
    bad = np.nonzero(kv.astype(np.uint64) != ekv)[0]
    assert bad.size == 0, (ctx, "kv", int(bad[0]), int(kv[bad[0]]), int(ekv[bad[0]]))
    bad = np.nonzero(blk.astype(np.int64) != np.array(exp[1], np.int64))[0]
    assert bad.size == 0, (ctx, "block", int(bad[0]), int(blk[bad[0]]), exp[1][bad[0]])
    bad = np.nonzero(fl.astype(np.int64) != np.array(exp[2], np.int64))[0]
    assert bad.size == 0, (ctx, "flags", int(bad[0]), int(fl[bad[0]]), exp[2][bad[0]])


def device_result(r):
    """A SeekResult as (kv uint64, block uint32, flags uint8) numpy arrays."""
    return (r.kv.cpu().numpy().view(np.uint64), r.block.cpu().numpy().view(np.uint32), r.flags.cpu().numpy())
