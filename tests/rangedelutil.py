"""Helpers of the range-deletion tests (tests/test_rangedel.py,
tests/test_rangedel_gpu.py).

`brute_cover` is a third statement of include/pebble_amd.h's rule, independent
of both implementations: per key, the maximum over the UNFRAGMENTED tombstones
that are visible and cover it.  `fragment` is a Python fragmenter (pinned by the
reference's rowblk_fragment_iter builds in tests/golden/range_del.json): it
turns a section's overlapping tombstones into a run.  `expected_visible_rd`
applies the cover to visibleutil.expected_visible by taking the covered KVs out
of the batch first: a range-deleted KV is an invisible KV everywhere."""
import functools
import json
import os
import random

import numpy as np

from mergeutil import C, D, T, crdb_key
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare
from pebble_amd.rowblk import Writer, make_trailer
from scanutil import result_kvs
from visibleutil import MAX, expected_visible, host_from_blocks

RANGEDEL = N.PBL_KIND_RANGEDEL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range_del.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def tomb_visible(seq, snapshot):
    return snapshot >= MAX or seq < snapshot


ALL = N.PBL_RANGEDEL_ALL


def brute_cover(tombs, key, comparer, snapshot=MAX, level=None):
    """max{t : (start, end, t) visible at the snapshot, start <= key < end}, or 0.
    With levels (tombstones (start, end, t, level), the key's `level`): ALL when
    such a tombstone with t > 0 lies in a shallower level than the key's."""
    hit = [x for x in tombs if tomb_visible(x[2], snapshot) and x[2] > 0 and key_compare(comparer, x[0], key) <= 0
           and key_compare(comparer, key, x[1]) < 0]
    if level is not None and any(x[3] < level for x in hit):
        return ALL
    return max((x[2] for x in hit), default=0)


def section_levels(define):
    """A level per section, smaller = shallower: memtables above L0 above L1 ...;
    among memtables and among L0 sections the one listed later is the newer,
    shallower one; sections of one deeper level share it."""
    def rank(i, s):
        name = s["level"]
        cls = -1 if name == "mem" else int(name[1:])
        return (cls, -i if cls <= 0 else 0)
    ranks = [rank(i, s) for i, s in enumerate(define["sections"])]
    order = sorted(set(ranks))
    return [order.index(r) for r in ranks]


def fragment(spans, comparer=D):
    """keyspan.Fragmenter over [(start, end, [key, ...])], a key being any tuple
    that starts with (seq, kind): [(start, end, [key, ...])] with every key of a
    fragment in trailer-descending order (stable), the fragments in start
    order.  Empty spans (start >= end) are dropped."""
    ck = functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b))
    spans = [s for s in spans if key_compare(comparer, s[0], s[1]) < 0]
    bounds = sorted({b for s, e, _ in spans for b in (s, e)}, key=ck)
    uniq = []
    for b in bounds:
        if not uniq or key_compare(comparer, uniq[-1], b) != 0:
            uniq.append(b)
    out = []
    for lo, hi in zip(uniq, uniq[1:]):
        keys = [k for s, e, ks in spans if key_compare(comparer, s, lo) <= 0 and key_compare(comparer, hi, e) <= 0
                for k in ks]
        if keys:
            keys.sort(key=lambda k: (-k[0], -k[1]))
            out.append((lo, hi, keys))
    return out


def run_kvs(tombs, comparer=D):
    """The KVs of a run, (start, trailer, end), from unfragmented (start, end, seq)."""
    return [(s, make_trailer(k[0], RANGEDEL), e) for s, e, ks in fragment([(s, e, [(t, RANGEDEL)]) for s, e, t in tombs],
                                                                          comparer) for k in ks]


def run_host(kvs):
    """A run as `to_host()` lays a decoded one-block batch out."""
    return host_from_blocks([kvs])


def run_block(kvs) -> bytes:
    """A row-format range-del block: restart interval 1 (rowblk_fragment_iter.go:116-139)."""
    w = Writer(1)
    for s, t, e in kvs:
        w.add(s, t, e)
    return w.finish()


def set_kvs(r):
    """[(boundary, cover)] of a set in to_host()'s layout."""
    assert all(v == b"" and f == 0 and t & 0xff == RANGEDEL for _, t, v, f in result_kvs(r, 0))
    return [(k, t >> 8) for k, t, _, _ in result_kvs(r, 0)]


def expected_set(runs, comparer, snapshot=MAX):
    """[(boundary, cover)] from the runs' KV lists (each (start, trailer, end)):
    the distinct boundaries in order, the bytes of the first in (run, fragment,
    start before end) order, the cover by brute force."""
    tombs = [(s, e, t >> 8) for kvs in runs for s, t, e in kvs]
    bs = [b for kvs in runs for s, _, e in kvs for b in (s, e)]
    bs.sort(key=functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b)))  # (stable)
    out = []
    for b in bs:
        if not out or key_compare(comparer, out[-1][0], b) != 0:
            out.append((b, brute_cover(tombs, b, comparer, snapshot)))
    return out


def expected_cover(runs, h, comparer, snapshot=MAX):
    """Per KV of the host batch `h`, brute force over the runs' fragments."""
    tombs = [(s, e, t >> 8) for kvs in runs for s, t, e in kvs]
    out = np.zeros(int(h["n_kv"]), np.uint64)
    for q in range(len(h["blk_status"])):
        if int(h["blk_status"][q]):
            continue
        kv0 = int(h["blk_kv_base"][q])
        for j, (k, _, _, _) in enumerate(result_kvs(h, q)):
            out[kv0 + j] = brute_cover(tombs, k, comparer, snapshot)
    return out


def expected_visible_rd(h, comparer, snapshot, keep, cover):
    """visibleutil.expected_visible with rule 1 extended by the cover: the
    statuses that do not depend on visibility come from the whole batch (a
    snapshot of 0 sees nothing), the results from the batch without the covered
    KVs, their src_kv mapped back."""
    base = expected_visible(h, comparer, 0, keep)
    blocks, maps = [], []
    for q, (st, _) in enumerate(base):
        if st:
            blocks.append([] if int(h["blk_status"][q]) == 0 else None)
            maps.append([])
            continue
        kv0 = int(h["blk_kv_base"][q])
        kvs = result_kvs(h, q)
        kept = [j for j, kv in enumerate(kvs) if not int(cover[kv0 + j]) > (kv[1] >> 8)]
        blocks.append([kvs[j] for j in kept])
        maps.append([kv0 + j for j in kept])
    h2 = host_from_blocks(blocks)
    out = []
    for q, (st, res) in enumerate(expected_visible(h2, comparer, snapshot, keep)):
        if base[q][0]:
            out.append((base[q][0], []))
            continue
        kv0 = int(h2["blk_kv_base"][q])
        out.append((st, [x[:4] + (maps[q][x[4] - kv0], x[5]) for x in res] if st == 0 else []))
    return out


def assert_visible_rd_is(res, exp, ctx=""):
    r, src_kv, n_src = res
    assert len(r["blk_status"]) == len(exp), ctx
    bad, mask = 0, 0
    for q, (st, e) in enumerate(exp):
        assert int(r["blk_status"][q]) == st, (ctx, q, int(r["blk_status"][q]), st)
        if st:
            bad += 1
            mask |= 1 << st
        kv0 = int(r["blk_kv_base"][q])
        got = result_kvs(r, q)
        assert [g[:2] for g in got] == [x[:2] for x in e], (ctx, q, [g[:2] for g in got], [x[:2] for x in e])
        assert got == [x[:4] for x in e], (ctx, q)
        assert np.asarray(src_kv[kv0: kv0 + len(e)]).tolist() == [x[4] for x in e], (ctx, q, "src_kv")
        assert np.asarray(n_src[kv0: kv0 + len(e)]).tolist() == [x[5] for x in e], (ctx, q, "n_src")
    assert r["n_kv"] == sum(len(e) for _, e in exp) and r["n_bad_blocks"] == bad and r["status_mask"] == mask, ctx


# ---- the reference's range_del cases ------------------------------------------------------------
def golden_sections(define, kinds):
    """Per section (point KVs sorted as a block, run KVs, unfragmented tombstones)."""
    out = []
    for s in define["sections"]:
        pts = [(k.encode(), make_trailer(seq, kinds[kind]), v.encode()) for k, seq, kind, v in s["kvs"] if kind != "RANGEDEL"]
        pts.sort(key=lambda kv: (kv[0], -kv[1]))
        tombs = [(k.encode(), v.encode(), seq) for k, seq, kind, v in s["kvs"] if kind == "RANGEDEL"]
        out.append((pts, run_kvs(tombs), tombs))
    return out


def replay_case(kvs, case):
    """The lines the reference prints for a `get` or `iter` case over the
    collapsed result [(key, value)]; a get is a seek-ge plus an equality test."""
    from visibleutil import replay
    if case["op"] == "iter":
        return replay(kvs, case["input"])
    d = dict(kvs)
    return ["%s:%s" % (k, d[k.encode()].decode()) if k.encode() in d else "%s: pebble: not found" % k for k in case["input"]]


# ---- generated runs -----------------------------------------------------------------------------
def gen_key(i, comparer=D, keylen=8):
    """Key number i, ascending in i under the comparer.  TESTKEYS and CRDB:
    three keys per prefix, the bare prefix and two versions."""
    if keylen == 1:
        assert comparer == D and i < 256
        return bytes([i])
    base = lambda x: b"k" * (keylen - 8) + b"%08d" % x  # noqa: E731
    if comparer == T:
        return base(i // 3) + (b"@%d" % (9 - i % 3) if i % 3 else b"")
    if comparer == C:
        return crdb_key(base(i // 3), 9 - i % 3) if i % 3 else crdb_key(base(i // 3))
    return base(i)


def random_runs(rng, n_runs, per_run, comparer=D, keylen=8, seq_hi=1000, shape="distinct"):
    """n_runs valid runs of per_run fragments each, as KV lists (start, trailer, end).
    shape: "distinct" all boundaries of all runs distinct, the runs interleaved
    in key space; "same_start" every fragment of a run has the same start and
    end; "shared" one key is an end and a start in every run."""
    key = lambda i: gen_key(i, comparer, keylen)  # noqa: E731
    tr = lambda: make_trailer(rng.randrange(1, seq_hi), RANGEDEL)  # noqa: E731
    runs = []
    for r in range(n_runs):
        if shape == "same_start":
            seqs = sorted(rng.sample(range(1, seq_hi), per_run), reverse=True)
            kvs = [(key(1), make_trailer(s, RANGEDEL), key(5 + r)) for s in seqs]
        elif shape == "shared":
            if per_run == 1:
                kvs = [(key(4990), tr(), key(5000)) if r % 2 else (key(5000), tr(), key(5010))]
            else:
                nlo = (per_run - 2) // 2
                nhi = per_run - 2 - nlo
                kvs = [(key(2 * i), tr(), key(2 * i + 1)) for i in range(nlo)]
                kvs += [(key(4990 - r), tr(), key(5000)), (key(5000), tr(), key(5010 + r))]
                kvs += [(key(6000 + 2 * i), tr(), key(6001 + 2 * i)) for i in range(nhi)]
        else:
            # fragment f of all n_runs * per_run, dealt round-robin: the runs interleave
            kvs = [(key(2 * f), tr(), key(2 * f + 1)) for f in range(r, n_runs * per_run, n_runs)]
        runs.append(kvs)
    return runs
