"""Helpers of the batched-scan tests (tests/test_scan.py, tests/test_scan_gpu.py):
the expected result of a bounded scan from the one-key host iterator
(pebble_amd.blockiter.DataIter), one block at a time, and exact comparisons of
every array of a scan result."""
import numpy as np

from pebble_amd import _native as N
from pebble_amd.blockiter import DataIter
from seekutil import CMP, trailer_index

ARRAYS = ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status", "trailer", "kv_flags",
          "key_off", "val_off", "key_bytes", "val_bytes")
TOTALS = ("n_kv", "key_bytes_total", "val_bytes_total", "n_restarts", "status_mask", "n_bad_blocks")


def expected_scan(h, lowers, uppers, comparer, blocks=None, hide=False, tidx=None):
    """Per query, the list of (source KV index, key, trailer, value, flags) that
    SetBounds(lower, upper); First(); Next()... returns: DataIter.SeekGE(lower)
    (First() for an empty or None lower), Next() until the key is >= upper under
    seekutil.CMP, then on to the next PBL_OK block.  None for a query whose
    named block is past n_blocks or not PBL_OK."""
    tidx = tidx if tidx is not None else trailer_index(h)
    cmp = CMP[comparer]
    nb = len(h["blk_status"])
    its = {}

    def it(b):
        if b not in its:
            its[b] = DataIter(h, b, comparer, hide)
        return its[b]

    out = []
    for i, (lo, up) in enumerate(zip(lowers, uppers)):
        if blocks is not None:
            b = int(blocks[i])
            if b >= nb or int(h["blk_status"][b]) != 0:
                out.append(None)
                continue
            order = [b]
        else:
            order = [b for b in range(nb) if int(h["blk_status"][b]) == 0]
        res, done = [], False
        for b in order:
            kv = it(b).SeekGE(lo) if lo else it(b).First()
            while kv is not None:
                if up is not None and cmp(kv.user_key, up) >= 0:
                    done = True
                    break
                src = tidx[(kv.user_key, kv.trailer)]
                res.append((src, kv.user_key, kv.trailer, kv.value, int(h["kv_flags"][src])))
                kv = it(b).Next()
            if done:
                break
        out.append(res)
    return out


def result_kvs(r, q):
    """(key, trailer, value, flags) of query q's KVs from a result in to_host()'s layout."""
    kv0, kv1 = int(r["blk_kv_base"][q]), int(r["blk_kv_base"][q + 1])
    ko = r["key_off"][kv0 + q: kv1 + q + 1].astype(np.int64)
    vo = r["val_off"][kv0 + q: kv1 + q + 1].astype(np.int64)
    kb, vb = int(r["blk_key_base"][q]), int(r["blk_val_base"][q])
    assert ko[0] == 0 and vo[0] == 0, (q, "offsets are relative to the query")
    return [(r["key_bytes"][kb + ko[j]: kb + ko[j + 1]].tobytes(), int(r["trailer"][kv0 + j]),
             r["val_bytes"][vb + vo[j]: vb + vo[j + 1]].tobytes(), int(r["kv_flags"][kv0 + j]))
            for j in range(kv1 - kv0)]


def assert_scan_is(res, exp, comparer, ctx=""):
    """A result (dict, range [n, 2], src_kv) against expected_scan()'s lists,
    and each query re-read through DataIter(result, q, comparer)."""
    r, rng, src = res
    n = len(exp)
    assert len(r["blk_status"]) == n and len(r["blk_kv_base"]) == n + 1, ctx
    bad = 0
    for q, e in enumerate(exp):
        kv0 = int(r["blk_kv_base"][q])
        if e is None:
            assert int(r["blk_status"][q]) != 0 and not result_kvs(r, q), (ctx, q)
            bad += 1
            continue
        assert int(r["blk_status"][q]) == 0, (ctx, q)
        got = result_kvs(r, q)
        assert got == [x[1:] for x in e], (ctx, q, len(got), len(e))
        assert src[kv0: kv0 + len(e)].tolist() == [x[0] for x in e], (ctx, q, "src_kv")
        lo, hi = int(rng[q][0]), int(rng[q][1])
        assert lo <= hi, (ctx, q)
        if e:  # the source range holds the result, and starts at its first KV when nothing was passed over
            assert lo <= e[0][0] and e[-1][0] < hi, (ctx, q, "range")
        it = DataIter(r, q, comparer)
        kv, k = it.First(), 0
        while kv is not None:
            assert (kv.user_key, kv.trailer, kv.value) == e[k][1:4], (ctx, q, k, "DataIter")
            kv, k = it.Next(), k + 1
        assert k == len(e), (ctx, q, "DataIter count")
    assert int(r["blk_kv_base"][n]) == r["n_kv"] == sum(len(e) for e in exp if e is not None), ctx
    assert int(r["blk_key_base"][n]) == r["key_bytes_total"] == len(r["key_bytes"]), ctx
    assert int(r["blk_val_base"][n]) == r["val_bytes_total"] == len(r["val_bytes"]), ctx
    assert r["n_bad_blocks"] == bad and (r["status_mask"] != 0) == (bad != 0), ctx
    assert not r["blk_rst_base"].any() and r["n_restarts"] == 0, ctx


def assert_same(a, b, ctx=""):
    """Two results (dict, range, src_kv), every array and total, exactly."""
    (ra, ga, sa), (rb, gb, sb) = a, b
    for k in ARRAYS:
        x, y = np.asarray(ra[k]), np.asarray(rb[k])
        assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k)
    for k in ("entry_off", "tiering_span_id", "tiering_attr"):
        if ra.get(k) is not None and rb.get(k) is not None:
            assert (np.asarray(ra[k]).astype(np.uint64) == np.asarray(rb[k]).astype(np.uint64)).all(), (ctx, k)
    for k in TOTALS:
        assert int(ra[k]) == int(rb[k]), (ctx, k, ra[k], rb[k])
    assert (np.asarray(ga).astype(np.uint64) == np.asarray(gb).astype(np.uint64)).all(), (ctx, "range")
    assert (np.asarray(sa).astype(np.uint64) == np.asarray(sb).astype(np.uint64)).all(), (ctx, "src_kv")


def device_result(res):
    """A ScanResult as (to_host() dict, range uint64 [n, 2], src_kv uint64) numpy."""
    return (res.batch.to_host(), res.range.cpu().numpy().view(np.uint64), res.src_kv.cpu().numpy().view(np.uint64))
