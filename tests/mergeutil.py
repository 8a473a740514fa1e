"""Helpers of the batched-merge tests (tests/test_merge.py, tests/test_merge_gpu.py).

The expectation is independent of both implementations: the (key, trailer,
value, flags) tuples of block q of every run under Python `sorted`, with a
`cmp_to_key` over pbl_key_compare, then trailer descending, then run, then
index.  The case list is shared: a case is a list of runs, a run a list of
blocks, a block a list of (user key, trailer, value) in the run's order, or None
for a block that is not PBL_OK.  test_merge.py lays the cases out as host
arrays directly; test_merge_gpu.py encodes them as row blocks and decodes those
on the device."""
import functools
import random
import struct

import numpy as np

from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare
from pebble_amd.rowblk import make_trailer
from scanutil import ARRAYS, TOTALS, result_kvs

D, T, C = N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB
BAD = N.PBL_CORRUPT_NO_RESTARTS  # the status of a None block


def S(seq):
    return make_trailer(seq, 1)


def ikey_cmp(comparer, a, b):
    """(key, trailer) pairs: base.InternalCompare."""
    c = key_compare(comparer, a[0], b[0])
    if c:
        return c
    return (a[1] < b[1]) - (a[1] > b[1])  # trailer descending


def host_from_blocks(blocks):
    """A run as `to_host()` lays a decoded batch out (kv_flags zero, no entry_off)."""
    nb = len(blocks)
    tr, ko, vo, kb, vb = [], [], [], bytearray(), bytearray()
    kvb, keyb, valb, st = [0], [0], [0], []
    for blk in blocks:
        k0, v0 = len(kb), len(vb)
        for k, t, v in (blk or []):
            ko.append(len(kb) - k0)
            vo.append(len(vb) - v0)
            tr.append(t)
            kb += k
            vb += v
        ko.append(len(kb) - k0)
        vo.append(len(vb) - v0)
        st.append(BAD if blk is None else 0)
        kvb.append(len(tr))
        keyb.append(len(kb))
        valb.append(len(vb))
    bad = sum(1 for s in st if s)
    return {"trailer": np.array(tr, np.uint64), "kv_flags": np.zeros(len(tr), np.uint8), "entry_off": None,
            "key_off": np.array(ko, np.uint32), "val_off": np.array(vo, np.uint32),
            "key_bytes": np.frombuffer(bytes(kb), np.uint8).copy(), "val_bytes": np.frombuffer(bytes(vb), np.uint8).copy(),
            "restarts": None, "blk_kv_base": np.array(kvb, np.uint64), "blk_key_base": np.array(keyb, np.uint64),
            "blk_val_base": np.array(valb, np.uint64), "blk_rst_base": np.zeros(nb + 1, np.uint64),
            "blk_status": np.array(st, np.uint32), "n_kv": len(tr), "key_bytes_total": len(kb),
            "val_bytes_total": len(vb), "n_restarts": 0, "status_mask": (1 << BAD) if bad else 0, "n_bad_blocks": bad,
            "n_slow_blocks": 0}


def expected_merge(hosts, comparer):
    """Per result block (status, [(key, trailer, value, flags, run, kv index in the run)])."""
    nb = len(hosts[0]["blk_status"])
    out = []
    for q in range(nb):
        st = next((int(h["blk_status"][q]) for h in hosts if int(h["blk_status"][q]) != 0), 0)
        items = []
        if st == 0:
            for r, h in enumerate(hosts):
                kvs = result_kvs(h, q)
                if any(ikey_cmp(comparer, kvs[j], kvs[j + 1]) > 0 for j in range(len(kvs) - 1)):
                    st = N.PBL_INVALID_ARG
                items += [(k, t, v, f, r, int(h["blk_kv_base"][q]) + j) for j, (k, t, v, f) in enumerate(kvs)]
        if st != 0:
            out.append((st, []))
            continue

        def order(a, b):
            return ikey_cmp(comparer, a, b) or (a[4] > b[4]) - (a[4] < b[4]) or (a[5] > b[5]) - (a[5] < b[5])

        out.append((0, sorted(items, key=functools.cmp_to_key(order))))
    return out


def assert_merge_is(res, hosts, comparer, ctx=""):
    """A result (dict, src_run, src_kv) against expected_merge()."""
    r, src_run, src_kv = res
    exp = expected_merge(hosts, comparer)
    n = len(exp)
    assert len(r["blk_status"]) == n and len(r["blk_kv_base"]) == n + 1, ctx
    bad, mask = 0, 0
    for q, (st, e) in enumerate(exp):
        assert int(r["blk_status"][q]) == st, (ctx, q, int(r["blk_status"][q]), st)
        if st:
            bad += 1
            mask |= 1 << st
        kv0 = int(r["blk_kv_base"][q])
        got = result_kvs(r, q)
        assert len(got) == len(e), (ctx, q, len(got), len(e))
        for j, (g, x) in enumerate(zip(got, e)):
            assert g == x[:4], (ctx, q, j, g[:2], x[:2])
        assert src_run[kv0: kv0 + len(e)].tolist() == [x[4] for x in e], (ctx, q, "src_run")
        assert src_kv[kv0: kv0 + len(e)].tolist() == [x[5] for x in e], (ctx, q, "src_kv")
    assert int(r["blk_kv_base"][n]) == r["n_kv"] == sum(len(e) for _, e in exp), ctx
    assert int(r["blk_key_base"][n]) == r["key_bytes_total"] == len(r["key_bytes"]), ctx
    assert int(r["blk_val_base"][n]) == r["val_bytes_total"] == len(r["val_bytes"]), ctx
    assert r["n_bad_blocks"] == bad and r["status_mask"] == mask, ctx
    assert not r["blk_rst_base"].any() and r["n_restarts"] == 0, ctx


def assert_same(a, b, ctx="", skip=()):
    """Two results (dict, src_run, src_kv): every array and total, exactly."""
    (ra, ua, sa), (rb, ub, sb) = a, b
    for k in ARRAYS + ("entry_off", "tiering_span_id", "tiering_attr"):
        if k in skip:
            continue
        x, y = ra.get(k), rb.get(k)
        assert (x is None) == (y is None), (ctx, k)
        if x is not None:
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k)
    for k in TOTALS:
        assert int(ra[k]) == int(rb[k]), (ctx, k, ra[k], rb[k])
    if "src" not in skip:
        assert np.asarray(ua).tolist() == np.asarray(ub).tolist(), (ctx, "src_run")
        assert np.asarray(sa).astype(np.uint64).tolist() == np.asarray(sb).astype(np.uint64).tolist(), (ctx, "src_kv")


def device_result(res):
    """A MergeResult as (to_host() dict, src_run uint8, src_kv uint64) numpy."""
    return (res.batch.to_host(), res.src_run.cpu().numpy(), res.src_kv.cpu().numpy().view(np.uint64))


# ---- the case list --------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257]


def _sorted_block(rng, n, seq0, n_keys=300):
    """n KVs with user keys drawn from a small pool (so runs share user keys),
    distinct sequence numbers, in (key ascending, trailer descending) order."""
    kvs = [(b"k%05d" % rng.randrange(n_keys), seq0 + i) for i in range(n)]
    kvs.sort(key=lambda x: (x[0], -x[1]))
    return [(k, S(s), b"v%d." % s + bytes([s & 0xff]) * (s % 7)) for k, s in kvs]


def crdb_key(roach, wall=None, logical=None, synthetic=False):
    if wall is None:
        return roach + b"\x00"
    if logical is None:
        return roach + b"\x00" + struct.pack(">Q", wall) + b"\x09"
    if not synthetic:
        return roach + b"\x00" + struct.pack(">QI", wall, logical) + b"\x0d"
    return roach + b"\x00" + struct.pack(">QI", wall, logical) + b"\x01\x0e"


def cases():
    """[(name, comparer, runs)]"""
    out = []
    rng = random.Random(1234)
    for K in (1, 2, 3, 16):  # run lengths around the wave and the tile, mixed in one batch of blocks
        runs = [[_sorted_block(rng, LENGTHS[(q + 3 * r) % 8], 100000 * r + 1000 * q + 1) for q in range(8)]
                for r in range(K)]
        out.append(("lengths K=%d" % K, D, runs))
    out.append(("every run empty", D, [[[], []] for _ in range(3)]))
    # one user key in every run, interleaved sequence numbers
    out.append(("one user key", D, [[[(b"same", S(s), b"r%d s%d" % (r, s)) for s in range(40 + r, r, -4)]]
                                    for r in range(4)]))
    # the identical (key, trailer) in three runs: run order decides
    tie = [[[(b"a", S(9), b"run%d a9" % r), (b"b", S(5), b"run%d b5 first" % r), (b"b", S(5), b"run%d b5 second" % r),
             (b"c", S(1), b"run%d" % r)]] for r in range(3)]
    out.append(("equal internal keys", D, tie))
    # testkeys: a@10 < a@5 under the comparer, the bare prefix first; "_synthetic" compares equal
    tk = [[[(b"a", S(3), b"r0 a"), (b"a@10", S(7), b"r0 a@10"), (b"a@5", S(7), b"r0 a@5"), (b"b@2", S(1), b"r0")]],
          [[(b"a@10", S(8), b"r1 a@10"), (b"a@5_synthetic", S(7), b"r1 a@5_synthetic"), (b"a@5", S(6), b"r1 a@5")]],
          [[(b"a", S(4), b"r2 a"), (b"a@7", S(2), b"r2 a@7"), (b"b", S(9), b"r2 b"), (b"b@2", S(1), b"r2 tie")]]]
    out.append(("testkeys suffixes", T, tk))
    # crdb: wall 5 as 8 bytes, as wall + zero logical, and with the synthetic bit compare equal
    ck = [[[(crdb_key(b"k1"), S(9), b"r0 bare"), (crdb_key(b"k1", 7), S(5), b"r0 7"), (crdb_key(b"k1", 5), S(5), b"r0 5"),
            (crdb_key(b"k2", 5, 3), S(2), b"r0 k2")]],
          [[(crdb_key(b"k1", 7, 1), S(5), b"r1 7,1"), (crdb_key(b"k1", 5, 0), S(6), b"r1 5,0"),
            (crdb_key(b"k1", 5, 0, True), S(5), b"r1 5,0,syn")]],
          [[(crdb_key(b"k1", 5, 0, True), S(5), b"r2 5,0,syn"), (crdb_key(b"k1", 5), S(4), b"r2 5"),
            (crdb_key(b"k2", 5, 3), S(2), b"r2 k2 tie")]]]
    out.append(("crdb equal versions", C, ck))
    # key lengths around the 16-B compare chunk, value lengths around every copy form
    klens, vlens = [0, 1, 15, 16, 17, 200], [0, 1, 15, 16, 17, 511, 512, 513, 5000]
    keys = sorted({(b"m" * kl)[:kl] for kl in klens} | {(b"m" * 15 + bytes([x]) + b"q" * 200)[:kl] for kl in klens
                                                        for x in (1, 2)})
    runs = []
    for r in range(2):
        blk = []
        for i, k in enumerate(keys):
            for j in range(2):
                s = 1000 - 10 * i - 2 * j - r
                vl = vlens[(3 * i + j + 4 * r) % len(vlens)]
                blk.append((k, S(s), bytes((s + t) & 0xff for t in range(vl))))
        runs.append([blk, blk[: 5 + r]])
    out.append(("key and value lengths", D, runs))
    # an unsorted block (run 1, block 1): its neighbours are merged
    good = [[_sorted_block(rng, 20 + q, 10000 * r + 100 * q + 1, 30) for q in range(3)] for r in range(2)]
    good[1][1] = good[1][1][::-1]
    out.append(("unsorted block", D, good))
    # trailers ascending within one user key are out of order too
    asc = [[[(b"x", S(1), b"old"), (b"x", S(2), b"new")]], [[(b"x", S(3), b"other")]]]
    out.append(("unsorted trailers", D, asc))
    # a block that is not PBL_OK in run 1
    runs = [[_sorted_block(rng, 10 + q, 10000 * r + 100 * q + 1, 30) for q in range(3)] for r in range(3)]
    runs[1][1] = None
    out.append(("bad block", D, runs))
    return out
