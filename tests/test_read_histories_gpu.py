"""pebble_amd.visible.read() on the device against the reference's recorded
iterator histories (tests/golden/iter_histories.json), against read()'s
composition over the host forms (readutil.read_host_forms, array for array) and
against the whole-path model (readutil.expected_read), in three table layouts;
then generated histories at the sizes where the kernels change behaviour, under
the three comparers.  tests/test_read_histories.py is the CPU half and states
the fixture's floors."""
import random

import numpy as np
import pytest

import readutil as R
from keyspanutil import assert_same
from pebble_amd.visible import read
from rangekeyutil import sets_of
from readutil import C, D, MAX, T, History, expected_read, read_host_forms, replay, result_points, result_spans, tables
from visibleutil import device_result

pytestmark = pytest.mark.gpu

G = R.load_golden()
GROUPS = R.groups(G)


def group_id(key):
    sec, n, mask = key
    return "%s-%d-w%d%s" % (G["sections"][sec]["file"], sec, n, "-mask" + mask if mask else "")


def user_spans(spans, comparer=T):
    return [(s, e, sets_of(ks, comparer)) for s, e, ks in spans]


def device_read(tabs, lo, up, snapshot=MAX, mask=None, keep=False, hide=False, ctx=""):
    """read() on the device == read_host_forms over to_host() of the same decoded
    inputs, every array and total.  Returns (points per range, spans per range)."""
    points, rk = read(tabs, lo, up, snapshot=snapshot, hide_obsolete_points=hide, keep_operands=keep, with_range_keys=True,
                      mask_suffix=mask)
    got, rkh = device_result(points), rk.to_host()
    want, wrk = read_host_forms(tabs, lo, up, snapshot=snapshot, hide_obsolete_points=hide, keep_operands=keep,
                                mask_suffix=mask)
    assert got[0]["status_mask"] == 0 and rkh["status_mask"] == 0, ctx
    assert_same(got[0], want[0], ctx, extras=False)
    assert got[1].tolist() == np.asarray(want[1]).tolist() and got[2].tolist() == np.asarray(want[2]).tolist(), ctx
    assert_same(rkh, wrk, ctx)
    n = len(lo)
    return [result_points(got[0], q) for q in range(n)], [result_spans(rkh, q) for q in range(n)]


def check_model(tabs, h, lo, up, snapshot=MAX, mask=None, keep=False, hide=False, ctx=""):
    """device_read(), and its result == the model's.  Returns the model's result."""
    pts, sps = device_read(tabs, lo, up, snapshot, mask, keep, hide, ctx)
    hidden = set().union(*[t.obsolete for t in tabs]) if hide else ()
    mp, ms = expected_read(h, lo, up, snapshot, mask, keep_operands=keep, hidden=hidden)
    for q in range(len(lo)):
        assert pts[q] == mp[q], (ctx, q, len(pts[q]), len(mp[q]))
        assert sps[q] == ms[q], (ctx, q)
    return mp, ms


# ---- 1. the recorded histories: one read() per (history, mask suffix), a range per segment ---------------
@pytest.mark.parametrize("key,segs", GROUPS, ids=[group_id(k) for k, _ in GROUPS])
def test_replay_recorded_segments(key, segs):
    sec, n_writes, mask = key
    h = History.from_fixture(G["sections"][sec], n_writes)
    lo, up, m = [R.b(s["lower"]) for s in segs], [R.b(s["upper"]) for s in segs], R.b(mask)
    want = [R.recorded(s["lines"]) for s in segs]
    first = None
    for layout in R.LAYOUTS:
        pts, sps = device_read(tables(h, layout, device=True), lo, up, mask=m, ctx=(key, layout))
        for q, s in enumerate(segs):
            got = replay(pts[q], user_spans(sps[q]), lo[q], R.b(s["start"]), len(s["lines"]))
            assert got == want[q], (layout, q, s["start"], got, want[q])
        first = first or (pts, sps)
        assert (pts, sps) == first, layout


def test_replay_bounded_iterator_cases():
    lines = 0
    for c in G["iterator"]:
        h = History.from_define(c["define"], G["kinds"], D)
        lo, up = [R.b(c["lower"])], [R.b(c["upper"])]
        want = R.recorded(c["lines"])
        for layout in ("one", "dealt"):
            pts, sps = device_read(tables(h, layout, device=True), lo, up, snapshot=c["seq"], ctx=(layout, c["lower"]))
            assert sps == [[]] and replay(pts[0], [], lo[0], R.b(c["start"]), len(want), D) == want, (layout, c)
        lines += len(want)
    assert lines >= 13


# ---- 2. result sizes around the wave and the tile, source blocks of 7, 64 and 130 KVs --------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("comparer", [D, T, C], ids=["default", "testkeys", "crdb"])
@pytest.mark.parametrize("per_block", [7, 64, 130])
def test_result_sizes(comparer, per_block):
    """Ranges [first key, key n) of a history of 300 keys hold exactly n KVs; a
    wide span, a tombstone over the last 20 keys and a newer version of every
    seventh key ride along.  Every range spans several source blocks."""
    bo = lambda i: R.bound_of(comparer, i)  # noqa: E731
    h = R.dense_history(comparer, 300, versions=(3, 2))
    h.write([("set", R.key_of(comparer, i, (3, 2)[i % 2]), b"newer%d" % i) for i in range(0, 300, 7)])
    h.write([("range-key-set", bo(10), bo(290), R.suffix_of(comparer, 3), b"wide"), ("del-range", bo(280), bo(300)),
             ("merge", R.key_of(comparer, 299, 3), b"over the tombstone")])
    lo, up = [None] * len(SIZES) + [bo(100)], [bo(n) for n in SIZES] + [None]
    tabs = tables(h, "dealt", device=True, per_block=per_block)
    for mask in (None, b"" if comparer == D else R.suffix_of(comparer, 3)):
        mp, ms = check_model(tabs, h, lo, up, mask=mask, ctx=(comparer, per_block, mask))
        if mask is None or comparer == D:
            assert [len(p) for p in mp] == list(SIZES) + [181]
        else:  # the keys with version 2 under the span are masked
            assert 0 < len(mp[-1]) < 181 and len(mp[0]) == 0 and len(mp[1]) == 1
        assert [len(s) for s in ms] == [0, 0, 1, 1, 1, 1, 1, 1, 1] and ms[-1][0][:2] == (bo(100), bo(290))


# ---- 3. 1, 2, 3 and 16 tables, some of them empty --------------------------------------------------------
@pytest.mark.parametrize("n_tables,n_ops", [(1, 120), (2, 120), (3, 120), (16, 120), (16, 9)])
def test_table_counts(n_tables, n_ops):
    rng = random.Random(n_tables * 1000 + n_ops)
    h = R.random_history(rng, T, n_keys=12, n_ops=n_ops, n_batches=n_tables + 4, p_range=0.2)
    tabs = tables(h, "dealt", device=True, n_tables=n_tables, per_block=7)
    empty = sum(1 for t in tabs if not t.points_host["n_kv"]), sum(1 for t in tabs if t.rd is None), \
        sum(1 for t in tabs if t.rk is None)
    if n_ops < n_tables:
        assert min(empty) > 0  # tables empty of points, of tombstones and of range keys
    lo, up = [None, R.bound_of(T, 3), R.bound_of(T, 8)], [None, R.bound_of(T, 9), R.bound_of(T, 8)]
    for snapshot in (MAX, R.SEQ0 + n_ops // 2):
        for mask in (None, b"@3"):
            check_model(tabs, h, lo, up, snapshot, mask, keep=mask is None, ctx=(n_tables, n_ops, snapshot, mask))
    batches = tables(h, "per_batch", device=True)
    assert len(batches) == min(h.n_batches, R.MAX_TABLES) and (n_ops < 100 or h.n_batches == n_tables + 4)
    check_model(batches, h, lo, up, MAX, b"@2", ctx=(n_tables, n_ops, "per_batch"))


# ---- 4. generated histories under the three comparers ----------------------------------------------------
def mask_of(comparer, version):
    return b"" if comparer == D else R.suffix_of(comparer, version)


@pytest.mark.parametrize("comparer", [D, T, C], ids=["default", "testkeys", "crdb"])
@pytest.mark.parametrize("seed,n_keys,n_ops,per_block", [(1, 24, 260, 64), (2, 40, 700, 7), (3, 200, 2500, 130)])
def test_generated_histories(comparer, seed, n_keys, n_ops, per_block):
    """Versions, tombstones and spans that collide: snapshots below, at and above
    the sequence numbers of a tombstone and of a range-key write, two mask
    suffixes and none, keep_operands on and off, hide_obsolete_points with
    obsolete rows; an unbounded side, an empty and an inverted range, bounds
    that tombstones and spans straddle."""
    rng = random.Random(100 * comparer + seed)
    h = R.random_history(rng, comparer, n_keys=n_keys, n_ops=n_ops, n_batches=5, p_range=0.12 if n_ops < 1000 else 0.03)
    bo = lambda i: R.bound_of(comparer, i)  # noqa: E731
    a, z = n_keys // 5, n_keys * 3 // 4
    lo = [None, bo(a), bo(a + 4), bo(z), None, R.key_of(comparer, a + 2, 2)]
    up = [None, bo(z), bo(a + 4), bo(a), bo(a + 6), None]
    t_seq, r_seq = h.tombs[len(h.tombs) // 2][2], h.rks[len(h.rks) // 2][2]
    layout = R.LAYOUTS[seed % 3]
    plain, marked = tables(h, layout, device=True, per_block=per_block), None
    masked = spans = hidden = 0
    for i, snapshot in enumerate((MAX, t_seq, t_seq + 1, r_seq, r_seq + 1, t_seq - 1)):
        for j, mask in enumerate((None, mask_of(comparer, 3), mask_of(comparer, 1))):
            keep, hide = (i + j) % 2 == 1, snapshot == MAX and j < 2
            if hide and marked is None:
                marked = tables(h, layout, device=True, per_block=per_block, mark_obsolete=True)
                hidden = sum(len(t.obsolete) for t in marked)
            mp, ms = check_model(marked if hide else plain, h, lo, up, snapshot, mask, keep, hide,
                                 (seed, snapshot, mask, keep, hide, layout))
            assert mp[2] == [] and mp[3] == [] and ms[2] == [] and ms[3] == []
            if mask is not None and snapshot == MAX:
                masked += expected_read(h, lo[:1], up[:1], snapshot, None, keep_operands=keep,
                                        hidden=set().union(*[t.obsolete for t in marked]) if hide else ())[0][0] != mp[0]
            spans += len(ms[0])
    assert spans > 0 and hidden > 0 and (comparer == D or masked > 0)


def test_interactions_by_hand():
    """tests/test_read_histories.py::test_interactions_by_hand's history on the
    device: a MERGE chain with a tombstoned and with a masked base, a point under
    a tombstone and a mask, a RANGEKEYDEL next to a del-range, spans across bounds."""
    h = History(T)
    h.write([("set", b"a@3", b"base;"), ("merge", b"a@3", b"m1;"), ("set", b"b@3", b"bbase;"), ("set", b"c@2", b"cbase;"),
             ("set", b"d@2", b"d;"), ("set", b"e", b"bare;"), ("set", b"f@9", b"above;"),
             ("set", b"h@5", b"hb;"), ("merge", b"h@5_synthetic", b"hs;")])
    h.write([("del-range", b"a", b"b"), ("merge", b"a@3", b"m2;"), ("merge", b"b@3", b"bm;"),
             ("range-key-set", b"b", b"e", b"@5", b"rk"), ("merge", b"c@2", b"cm;"), ("del-range", b"c", b"d"),
             ("range-key-set", b"e", b"g", b"@5", b"rk2"), ("range-key-del", b"f", b"g"), ("del-range", b"f", b"g"),
             ("singledel", b"d@2"), ("merge", b"h@5", b"hm;"), ("range-key-set", b"h", b"i", b"@5", b"rk3")])
    lo, up = [None, b"b@3", b"a"], [None, b"f", b"c"]
    for layout in R.LAYOUTS:
        tabs = tables(h, layout, device=True)
        plain, spans = check_model(tabs, h, lo, up, ctx=layout)
        assert [(k, v) for k, _, v in plain[0]] == [(b"a@3", b"m2;"), (b"b@3", b"bbase;bm;"), (b"e", b"bare;"),
                                                        (b"h@5", b"hb;hs;hm;")]
        assert [(s, e) for s, e, _ in spans[0]] == [(b"b", b"e"), (b"e", b"f"), (b"h", b"i")]
        assert [(s, e) for s, e, _ in spans[1]] == [(b"b@3", b"e"), (b"e", b"f")]
        for keep in (False, True):
            got, _ = check_model(tabs, h, lo, up, mask=b"@9", keep=keep, ctx=(layout, keep))
            # (h@5_synthetic, the middle operand of h@5's chain, is masked and skipped; the base below it is not)
            tail = [(b"h@5", b"hm;"), (b"h@5", b"hb;")] if keep else [(b"h@5", b"hb;hm;")]
            assert [(k, v) for k, _, v in got[0]] == [(b"a@3", b"m2;"), (b"e", b"bare;")] + tail
        for snapshot in sorted({r[2] for r in h.rks} | {t[2] for t in h.tombs}):
            for s in (snapshot - 1, snapshot, snapshot + 1):
                check_model(tabs, h, lo, up, s, b"@9", ctx=(layout, s))
