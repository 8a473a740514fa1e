"""read()'s composition against the reference's recorded iterator histories
(tests/golden/iter_histories.json, from testdata/iter_histories/* and the
bounded cases of testdata/iterator; tests/golden/make_read_fixtures.py states
the selection rules).  Every forward segment is replayed twice: through
readutil.read_host_forms (read()'s composition over the host forms) and
through readutil.expected_read (the whole-path model), each interleaved into the
combined stream and compared with the recorded lines, in all three table
layouts.  Generated histories then compare the host forms with the model at
the three comparers.  No device is needed; tests/test_read_histories_gpu.py
runs the same replay through read() itself."""
import random

import pytest

import readutil as R
from rangekeyutil import sets_of
from readutil import C, D, MAX, T, History, expected_read, read_host_forms, replay, result_points, result_spans, tables

G = R.load_golden()
GROUPS = R.groups(G)


def group_id(key):
    sec, n, mask = key
    return "%s-%d-w%d%s" % (G["sections"][sec]["file"], sec, n, "-mask" + mask if mask else "")


def has_op(seg, *names):
    writes = G["sections"][seg["section"]]["writes"][: seg["n_writes"]]
    return any(op[0] in names for w in writes for op in w.get("ops", []))


def user_spans(spans, comparer=T):
    """Spans reduced to what RangeKeys() reports: (start, end, the sets in suffix order)."""
    return [(s, e, sets_of(ks, comparer)) for s, e, ks in spans]


# ---- 1. the fixture holds what the issue counted ----------------------------------------------------------
def test_fixture_floors():
    segs = G["segments"]
    lines = [ln for s in segs for ln in s["lines"]]
    assert len(segs) >= 100 and len(lines) >= 170
    assert sum(1 for s in segs if s["mask_suffix"] is not None) >= 10
    assert sum(1 for ln in lines if ln is not None and ln[2] is not None) >= 60
    assert sum(1 for s in segs if has_op(s, "del-range")) >= 3
    assert sum(1 for s in segs if has_op(s, "range-key-set", "range-key-unset", "range-key-del")) >= 80
    assert any(has_op(s, "del", "singledel") for s in segs)
    assert any(s["lower"] for s in segs) and any(s["upper"] for s in segs)
    x = G["excluded"]
    assert x["scripts_taken"] >= 70 and x["scripts"] == x["scripts_taken"] + sum(
        x[k] for k in ("scripts_on_a_tainted_history", "scripts_with_another_option", "scripts_whose_lines_do_not_correspond",
                       "scripts_without_a_forward_segment"))
    assert len(G["iterator"]) >= 12 and sum(len(c["lines"]) for c in G["iterator"]) >= 13
    assert sum(len(v) for _, v in GROUPS) == len(segs)  # the replay below leaves no segment out


# ---- 2. the replay: host forms and model against the recorded lines, three layouts -------------------------
@pytest.mark.parametrize("key,segs", GROUPS, ids=[group_id(k) for k, _ in GROUPS])
def test_replay_recorded_segments(key, segs):
    sec, n_writes, mask = key
    h = History.from_fixture(G["sections"][sec], n_writes)
    lo, up, m = [R.b(s["lower"]) for s in segs], [R.b(s["upper"]) for s in segs], R.b(mask)
    want = [R.recorded(s["lines"]) for s in segs]
    model_p, model_s = expected_read(h, lo, up, mask_suffix=m)
    for q, s in enumerate(segs):
        got = replay(model_p[q], user_spans(model_s[q]), lo[q], R.b(s["start"]), len(s["lines"]))
        assert got == want[q], ("model", q, s["start"], got, want[q])
    first = None
    for layout in R.LAYOUTS:
        (r, _, _), rk = read_host_forms(tables(h, layout), lo, up, mask_suffix=m)
        assert r["status_mask"] == 0 and rk["status_mask"] == 0
        pts = [result_points(r, q) for q in range(len(segs))]
        sps = [result_spans(rk, q) for q in range(len(segs))]
        for q, s in enumerate(segs):
            got = replay(pts[q], user_spans(sps[q]), lo[q], R.b(s["start"]), len(s["lines"]))
            assert got == want[q], (layout, q, s["start"], got, want[q])
        # the layouts give identical points (keys, trailers, values) and identical range-key batches,
        # and they are the model's
        if first is None:
            first = (pts, sps)
            assert pts == model_p and sps == model_s, layout
        assert (pts, sps) == first, layout


# ---- 3. testdata/iterator's bounded cases, at their seq ---------------------------------------------------
def test_replay_bounded_iterator_cases():
    lines = 0
    for c in G["iterator"]:
        h = History.from_define(c["define"], G["kinds"], D)
        lo, up = [R.b(c["lower"])], [R.b(c["upper"])]
        want = R.recorded(c["lines"])
        mp, ms = expected_read(h, lo, up, snapshot=c["seq"])
        assert replay(mp[0], ms[0], lo[0], R.b(c["start"]), len(want), D) == want, ("model", c)
        for layout in R.LAYOUTS:
            (r, _, _), rk = read_host_forms(tables(h, layout), lo, up, snapshot=c["seq"])
            assert result_points(r, 0) == mp[0] and result_spans(rk, 0) == [], (layout, c)
            assert replay(result_points(r, 0), [], lo[0], R.b(c["start"]), len(want), D) == want, (layout, c)
        lines += len(want)
    assert lines >= 13


# ---- 4. generated histories: the host forms against the model ---------------------------------------------
def check_host_forms(h, layout, lo, up, snapshot, mask, keep, ctx, n_tables=3, per_block=64):
    (r, _, n_src), rk = read_host_forms(tables(h, layout, n_tables=n_tables, per_block=per_block), lo, up, snapshot=snapshot,
                                        keep_operands=keep, mask_suffix=mask)
    mp, ms = expected_read(h, lo, up, snapshot, mask, keep_operands=keep)
    assert r["status_mask"] == 0 and rk["status_mask"] == 0, ctx
    for q in range(len(lo)):
        assert result_points(r, q) == mp[q], (ctx, q)
        assert result_spans(rk, q) == ms[q], (ctx, q)
    return mp, ms


def mask_of(comparer, version):
    return b"" if comparer == D else R.suffix_of(comparer, version)


@pytest.mark.parametrize("comparer", [D, T, C], ids=["default", "testkeys", "crdb"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generated_histories(comparer, seed):
    rng = random.Random(100 * comparer + seed)
    h = R.random_history(rng, comparer, n_keys=24, n_ops=260, n_batches=5, p_range=0.12)
    bo = lambda i: R.bound_of(comparer, i)  # noqa: E731
    lo = [None, bo(5), bo(9), bo(12), None, R.key_of(comparer, 7, 2)]
    up = [None, bo(17), bo(9), bo(3), bo(11), None]
    t_seq, r_seq = h.tombs[len(h.tombs) // 2][2], h.rks[len(h.rks) // 2][2]
    masked = spans = 0
    for snapshot in (MAX, t_seq, t_seq + 1, r_seq, r_seq + 1, t_seq - 1):
        for mask in (None, mask_of(comparer, 3), mask_of(comparer, 1)):
            keep = (snapshot + len(mask or b"x")) % 2 == 1
            layout = R.LAYOUTS[(snapshot + seed) % 3]
            mp, ms = check_host_forms(h, layout, lo, up, snapshot, mask, keep, (seed, snapshot, mask, keep, layout))
            assert mp[2] == [] and mp[3] == [] and ms[2] == [] and ms[3] == []  # the empty and the inverted range
            if mask is not None and snapshot == MAX:
                plain = expected_read(h, lo, up, snapshot, None, keep_operands=keep)[0]
                masked += plain[0] != mp[0]
            spans += len(ms[0])
    assert spans > 0 and (comparer == D or masked > 0)  # (the default comparer's keys have no suffix: nothing is masked)


def test_interactions_by_hand():
    """The interactions the stages do not meet alone, each against the model
    and with its outcome spelled out."""
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
        plain, spans = check_host_forms(h, layout, lo, up, MAX, None, False, layout)
        # a MERGE chain whose base is tombstoned: only the operand above the tombstone is left
        assert [(k, v) for k, _, v in plain[0]] == [(b"a@3", b"m2;"), (b"b@3", b"bbase;bm;"), (b"e", b"bare;"),
                                                        (b"h@5", b"hb;hs;hm;")]
        # a RANGEKEYDEL next to a del-range: [f, g) lost its range key and its point
        assert [(s, e) for s, e, _ in spans[0]] == [(b"b", b"e"), (b"e", b"f"), (b"h", b"i")]
        # a span and a tombstone that cross a scan bound
        assert [(s, e) for s, e, _ in spans[1]] == [(b"b@3", b"e"), (b"e", b"f")]
        assert [(s, e) for s, e, _ in spans[2]] == [(b"b", b"c")] and [k for k, _, _ in plain[2]] == [b"a@3", b"b@3"]
        # masked at @9: b@3 (a whole MERGE chain, base and operand) and c@2 (also under a tombstone) go;
        # a@3 lies outside every span, e has no suffix.  h@5_synthetic is the same user key as h@5 and
        # another range-key suffix, after @5: the middle operand of h@5's chain is masked and skipped, the
        # operand above it and the base below it are not
        got, _ = check_host_forms(h, layout, lo, up, MAX, b"@9", False, layout)
        assert [(k, v) for k, _, v in got[0]] == [(b"a@3", b"m2;"), (b"e", b"bare;"), (b"h@5", b"hb;hm;")]
        kept, _ = check_host_forms(h, layout, lo, up, MAX, b"@9", True, layout)
        assert [(k, v) for k, _, v in kept[0]] == [(b"a@3", b"m2;"), (b"e", b"bare;"), (b"h@5", b"hm;"), (b"h@5", b"hb;")]
        # below the range-key set's sequence number nothing is masked; below the tombstones nothing is deleted
        rk_seq = next(r[2] for r in h.rks if r[0] == b"b")
        old, sp = check_host_forms(h, layout, lo, up, rk_seq, b"@9", False, layout)
        assert sp[0] == [] and [(k, v) for k, _, v in old[0]][:2] == [(b"a@3", b"m2;"), (b"b@3", b"bbase;bm;")]
        first, _ = check_host_forms(h, layout, lo, up, h.tombs[0][2], b"@9", False, layout)
        assert [(k, v) for k, _, v in first[0]][0] == (b"a@3", b"base;m1;")
