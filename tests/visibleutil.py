"""Helpers of the snapshot-visible tests (tests/test_visible.py,
tests/test_visible_gpu.py).

`expected_visible` is a third statement of include/pebble_amd.h's rules,
independent of both implementations: group by pbl_key_compare == 0, filter by
the snapshot, apply the head and chain rules.  The case list is shared: a case
is (name, comparer, blocks, snapshots); a block is a list of (user key, trailer,
value[, kv_flags]) in order, or None for a block that is not PBL_OK.
test_visible.py lays the cases out as host arrays directly; test_visible_gpu.py
encodes them as row blocks and decodes those on the device."""
import json
import os

import numpy as np

from mergeutil import BAD, C, D, T, crdb_key, ikey_cmp
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare
from pebble_amd.rowblk import make_trailer
from scanutil import ARRAYS, TOTALS, result_kvs

MAX = N.PBL_SEQNUM_MAX
DEL, SET, MERGE, SINGLEDEL, SETWITHDEL, DELSIZED = 0, 1, 2, 7, 18, 23
SETS, DELS = (SET, SETWITHDEL), (DEL, SINGLEDEL, DELSIZED)
HANDLES = N.PBL_KV_VALBLK_HANDLE | N.PBL_KV_BLOB_HANDLE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iterator_points.json")


def tr(seq, kind=SET):
    return make_trailer(seq, kind)


def host_from_blocks(blocks):
    """A batch as `to_host()` lays a decoded batch out (no entry_off)."""
    nb = len(blocks)
    t, fl, ko, vo, kb, vb = [], [], [], [], bytearray(), bytearray()
    kvb, keyb, valb, st = [0], [0], [0], []
    for blk in blocks:
        k0, v0 = len(kb), len(vb)
        for kv in (blk or []):
            ko.append(len(kb) - k0)
            vo.append(len(vb) - v0)
            t.append(kv[1])
            fl.append(kv[3] if len(kv) > 3 else 0)
            kb += kv[0]
            vb += kv[2]
        ko.append(len(kb) - k0)
        vo.append(len(vb) - v0)
        st.append(BAD if blk is None else 0)
        kvb.append(len(t))
        keyb.append(len(kb))
        valb.append(len(vb))
    bad = sum(1 for s in st if s)
    return {"trailer": np.array(t, np.uint64), "kv_flags": np.array(fl, np.uint8), "entry_off": None,
            "key_off": np.array(ko, np.uint32), "val_off": np.array(vo, np.uint32),
            "key_bytes": np.frombuffer(bytes(kb), np.uint8).copy(), "val_bytes": np.frombuffer(bytes(vb), np.uint8).copy(),
            "restarts": None, "blk_kv_base": np.array(kvb, np.uint64), "blk_key_base": np.array(keyb, np.uint64),
            "blk_val_base": np.array(valb, np.uint64), "blk_rst_base": np.zeros(nb + 1, np.uint64),
            "blk_status": np.array(st, np.uint32), "n_kv": len(t), "key_bytes_total": len(kb),
            "val_bytes_total": len(vb), "n_restarts": 0, "status_mask": (1 << BAD) if bad else 0, "n_bad_blocks": bad,
            "n_slow_blocks": 0}


def visible_at(trailer, snapshot):
    return snapshot >= MAX or (trailer >> 8) < snapshot


def expected_visible(h, comparer, snapshot=MAX, keep=False):
    """Per result block (status, [(key, trailer, value, flags, src_kv, n_src)])."""
    out = []
    for q in range(len(h["blk_status"])):
        st = int(h["blk_status"][q])
        kvs = result_kvs(h, q) if st == 0 else []
        kv0 = int(h["blk_kv_base"][q])
        if any(ikey_cmp(comparer, kvs[j], kvs[j + 1]) > 0 for j in range(len(kvs) - 1)):
            st = N.PBL_INVALID_ARG
        elif any((t & 0xff) not in SETS + DELS + (MERGE,) or f & N.PBL_KV_INVALID_KEY for _, t, _, f in kvs):
            st = N.PBL_UNSUPPORTED
        res, j = [], 0
        while st == 0 and j < len(kvs):
            e = j + 1
            while e < len(kvs) and key_compare(comparer, kvs[e - 1][0], kvs[e][0]) == 0:
                e += 1
            vis = [x for x in range(j, e) if visible_at(kvs[x][1], snapshot)]
            j = e
            if not vis or (kvs[vis[0]][1] & 0xff) in DELS:
                continue
            chain = [vis[0]]
            if (kvs[vis[0]][1] & 0xff) == MERGE:
                for x in vis[1:]:
                    kind = kvs[x][1] & 0xff
                    if kind in DELS:
                        break
                    chain.append(x)
                    if kind in SETS:
                        break
            if keep:
                res += [(kvs[x][0], kvs[x][1], kvs[x][2], kvs[x][3] & HANDLES, kv0 + x, len(chain) if i == 0 else 0)
                        for i, x in enumerate(chain)]
                continue
            if len(chain) > 1 and any(kvs[x][3] & HANDLES for x in chain):
                st = N.PBL_UNSUPPORTED
                break
            k, t, _, f = kvs[chain[0]]
            res.append((k, t, b"".join(kvs[x][2] for x in reversed(chain)), f & HANDLES, kv0 + chain[0], len(chain)))
        out.append((st, res if st == 0 else []))
    return out


def assert_visible_is(res, h, comparer, snapshot, keep, ctx=""):
    """A result (dict, src_kv, n_src) against expected_visible()."""
    r, src_kv, n_src = res
    exp = expected_visible(h, comparer, snapshot, keep)
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
            assert g == x[:4], (ctx, q, j, g[:2], x[:2], len(g[2]), len(x[2]))
        assert np.asarray(src_kv[kv0: kv0 + len(e)]).tolist() == [x[4] for x in e], (ctx, q, "src_kv")
        assert np.asarray(n_src[kv0: kv0 + len(e)]).tolist() == [x[5] for x in e], (ctx, q, "n_src")
    assert int(r["blk_kv_base"][n]) == r["n_kv"] == sum(len(e) for _, e in exp), ctx
    assert int(r["blk_key_base"][n]) == r["key_bytes_total"] == len(r["key_bytes"]), ctx
    assert int(r["blk_val_base"][n]) == r["val_bytes_total"] == len(r["val_bytes"]), ctx
    assert r["n_bad_blocks"] == bad and r["status_mask"] == mask, ctx
    assert not r["blk_rst_base"].any() and r["n_restarts"] == 0, ctx
    return exp


def assert_same(a, b, ctx=""):
    """Two results (dict, src_kv, n_src): every array and total, exactly."""
    (ra, sa, na), (rb, sb, nb) = a, b
    for k in ARRAYS + ("entry_off", "tiering_span_id", "tiering_attr"):
        x, y = ra.get(k), rb.get(k)
        assert (x is None) == (y is None), (ctx, k)
        if x is not None:
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k)
    for k in TOTALS:
        assert int(ra[k]) == int(rb[k]), (ctx, k, ra[k], rb[k])
    assert np.asarray(sa).astype(np.uint64).tolist() == np.asarray(sb).astype(np.uint64).tolist(), (ctx, "src_kv")
    assert np.asarray(na).astype(np.uint64).tolist() == np.asarray(nb).astype(np.uint64).tolist(), (ctx, "n_src")


def device_result(res):
    """A VisibleResult as (to_host() dict, src_kv uint64, n_src uint32) numpy."""
    return (res.batch.to_host(), res.src_kv.cpu().numpy().view(np.uint64), res.n_src.cpu().numpy().view(np.uint32))


def fold(exp_keep):
    """KEEP_OPERANDS results of one block folded as the default mode does: a
    chain's first KV (n_src > 0) takes the values of its n_src KVs, oldest first."""
    out, j = [], 0
    while j < len(exp_keep):
        k, t, _, f, s, n = exp_keep[j]
        assert n >= 1
        out.append((k, t, b"".join(x[2] for x in reversed(exp_keep[j: j + n])), f, s, n))
        j += n
    return out


# ---- the case list --------------------------------------------------------------------------
VALUE_LENGTHS = [0, 1, 15, 16, 17, 511, 512, 513, 5000]
KIND_CYCLE = [SET, MERGE, DEL, MERGE, SETWITHDEL, SINGLEDEL, MERGE, DELSIZED]


def group(key, n, seq0, kinds, val=lambda s: b"v%d," % s):
    """n versions of one key, sequence numbers seq0 + n - 1 down to seq0."""
    return [(key, tr(seq0 + n - 1 - i, kinds[i % len(kinds)]), val(seq0 + n - 1 - i)) for i in range(n)]


def edges_block():
    """Group boundaries at flat positions 63 / 64 / 65 and 255 / 256 / 257."""
    sizes, blk = [63, 1, 1, 190, 1, 1, 43], []
    for g, n in enumerate(sizes):
        kinds = KIND_CYCLE[g:] + KIND_CYCLE[:g]
        blk += group(b"g%02d" % g, n, 1000 * g + 1, kinds if g % 2 else [MERGE] * (n - 1) + [SET])
    assert len(blk) == 300
    return blk


def long_chain_block():
    """MERGE chains of 700 operands ending in a SET, in a DEL and at the block's end."""
    one = lambda s: bytes([s % 251])  # noqa: E731
    a = group(b"a", 700, 11, [MERGE] * 699 + [SET], one) + group(b"a", 2, 1, [SET], one)
    b = group(b"b", 701, 11, [MERGE] * 700 + [DEL], one) + group(b"b", 1, 1, [SET], one)
    c = group(b"c", 700, 11, [MERGE], one)
    return a + b + c


def one_key_block(n=70000):
    """One user key: n - 1 MERGE over one SET, 1-byte values that encode the position."""
    return group(b"the key", n, 1, [MERGE] * (n - 1) + [SET], lambda s: bytes([s % 251]))


def sweep_blocks():
    blocks, seq = [], 1
    for q in range(3):
        blk = []
        for g in range(12 + q):
            n = 1 + (5 * g + q) % 6
            blk += group(b"s%d-%02d" % (q, g), n, seq, KIND_CYCLE[(g + q) % 8:] + KIND_CYCLE[:(g + q) % 8])
            seq += n
        blocks.append(blk)
    return blocks, seq


def value_blocks():
    val = lambda i, n: bytes((i + t) & 0xff for t in range(n))  # noqa: E731
    heads = [(b"h%02d" % i, tr(50 + i), val(i, n)) for i, n in enumerate(VALUE_LENGTHS)]
    ops = [(b"chain", tr(100 - i, MERGE), val(40 + i, n)) for i, n in enumerate(VALUE_LENGTHS + VALUE_LENGTHS[::-1])]
    return [heads, ops, ops[:9] + [(b"chain", tr(5, SET), val(7, 513))] + heads]


def status_blocks():
    good = lambda q: (group(b"k%da" % q, 3, 10, [MERGE, MERGE, SET]) + group(b"k%db" % q, 2, 20, [DEL, SET])  # noqa: E731
                      + group(b"k%dc" % q, 1, 30, [SET]))
    unsorted = [(b"b", tr(2), b"x"), (b"a", tr(1), b"y")]
    ascending = [(b"x", tr(1), b"old"), (b"x", tr(2), b"new")]
    kind21 = [(b"a", tr(9), b"ok"), (b"b", tr(8, 21), b"range key set"), (b"c", tr(7), b"ok")]
    kind3 = [(b"a", tr(9, 3), b"log data")]
    handle = [(b"a", tr(9, MERGE), b"op"), (b"a", tr(8, SET), b"\x80handle", N.PBL_KV_VALBLK_HANDLE),
              (b"b", tr(7, SET), b"\x80alone", N.PBL_KV_BLOB_HANDLE)]
    invalid = [(b"a", tr(9), b"ok"), (b"b", tr(8), b"a key shorter than its trailer", N.PBL_KV_INVALID_KEY)]
    blocks = [good(0)]
    for q, b in enumerate((None, unsorted, ascending, kind21, kind3, invalid, handle)):
        blocks += [b, good(q + 1)]
    return blocks


def cases():
    """[(name, comparer, blocks, snapshots)]"""
    out = [("wave and tile edges", D, [edges_block(), edges_block()[:257]], [MAX, 2500])]
    long_inv = (group(b"a", 2, 3, [SET]) + group(b"inv", 600, 1001, KIND_CYCLE) + [(b"inv", tr(5), b"seen")]
                + group(b"z", 3, 6, [MERGE, MERGE, SET]))
    out.append(("long invisible prefix", D, [long_inv], [1000, MAX]))
    out.append(("long chains", D, [long_chain_block()], [MAX, 400]))
    blocks, seq = sweep_blocks()
    out.append(("snapshot sweep", D, blocks, [0, 1, seq // 2, MAX]))
    same = [group(b"a", 2, 1, [SET]) + group(b"same", 2, 8, [MERGE]), group(b"same", 2, 5, [MERGE, SET]) + group(b"t", 1, 1, [DEL])]
    out.append(("block independence", D, same, [MAX]))
    out.append(("empty blocks", D, [[], group(b"a", 1, 1, [SET]), [], []], [MAX]))
    out.append(("no blocks", D, [], [MAX]))
    out.append(("no KVs", D, [[], []], [MAX]))
    tk = [[(b"a@5", tr(9, MERGE), b"newest"), (b"a@5_synthetic", tr(7, MERGE), b"middle"), (b"a@5_synthetic", tr(3), b"oldest"),
           (b"b@2", tr(4, DEL), b""), (b"b@2_synthetic", tr(2), b"shadowed under testkeys")]]
    out.append(("testkeys equal suffixes", T, tk, [MAX, 8]))
    out.append(("testkeys inputs, default comparer", D, tk, [MAX, 8]))
    ck = [[(crdb_key(b"k1", 5, 0, True), tr(9, MERGE), b"syn"), (crdb_key(b"k1", 5, 0), tr(8, MERGE), b"zero logical"),
           (crdb_key(b"k1", 5), tr(7), b"wall only"), (crdb_key(b"k2", 5, 3), tr(2), b"k2")]]
    out.append(("crdb equal versions", C, ck, [MAX, 9]))
    out.append(("crdb inputs, default comparer", D, ck, [MAX, 9]))
    out.append(("value lengths", D, value_blocks(), [MAX]))
    out.append(("statuses", D, status_blocks(), [MAX]))
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_block(case, kinds):
    return [(k.encode(), tr(s, kinds[kind]), v.encode()) for k, s, kind, v in case["define"]]


def replay(kvs, commands):
    """The commands over the collapsed result [(key, value)] with a cursor:
    the lines the reference's iterator test prints."""
    lines, pos, n = [], -1, len(kvs)
    for c in commands:
        w = c.split()
        if w[0] == "first":
            pos = 0
        elif w[0] == "last":
            pos = n - 1
        elif w[0] == "next":
            pos = min(pos + 1, n)
        elif w[0] == "prev":
            pos = max(pos - 1, -1)
        elif w[0] == "seek-ge":
            pos = next((i for i, (k, _) in enumerate(kvs) if k >= w[1].encode()), n)
        elif w[0] == "seek-lt":
            pos = max((i for i, (k, _) in enumerate(kvs) if k < w[1].encode()), default=-1)
        else:
            raise AssertionError(c)
        lines.append("%s: (%s, .)" % (kvs[pos][0].decode(), kvs[pos][1].decode()) if 0 <= pos < n else ".")
    return lines
