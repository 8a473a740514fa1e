"""Range keys in the read path, the host forms (pebble_amd/csrc/rangekey.hip;
DESIGN.md §3.16): pbl_rangekey_set_host, pbl_rangekey_clip_host,
pbl_rangekey_mask_set_host and pbl_rangekey_mask_host against the Python
statement of the rules in rangekeyutil.py, byte for byte on every array and
total; that statement against the reference's data (tests/golden/rangekey.json)."""
import ctypes
import functools
import random

import numpy as np
import pytest

import rangekeyutil as U
from keyspanutil import assert_same, sized
from pebble_amd import _native as N
from pebble_amd.batch import Capacity, DecodeError
from pebble_amd.rangekey import build_set_host, clip_host, mask_host, mask_set_host, suffix_compare
from rangekeyutil import ALL, C, D, DEL, MAX, SET, T, UNSET, tr
from visibleutil import host_from_blocks

G = U.load_golden()
CASES = U.cases()


def host_set(runs, comparer, snapshot=MAX, **kw):
    return build_set_host([U.run_host(r) for r in runs], comparer, snapshot, **kw)


def check_set(runs, comparer, snapshot=MAX, ctx=""):
    exp = U.expected_spans(runs, comparer, snapshot)
    got = host_set(runs, comparer, snapshot)
    assert_same(got, U.layout([exp]), (ctx, snapshot))
    return exp, got


def point_batch(keys, per_block=50):
    """A host batch of point KVs (one SET per key) in blocks of per_block."""
    blocks = [[(k, 7 << 8 | 1, b"v") for k in keys[i: i + per_block]] for i in range(0, len(keys), per_block)]
    return host_from_blocks(blocks or [[]])


# ---- 1. CompareRangeSuffixes ------------------------------------------------------------------------------
def test_suffix_compare():
    pools = {
        D: [b"", b"a", b"ab", b"b", b"@5", b"\xff"],
        T: [b"", b"_synthetic", b"@5", b"@05", b"@5_synthetic", b"@7", b"@10", b"@0", b"@100_synthetic"],
        C: [b"", b"\x01", (5).to_bytes(8, "big") + b"\x09", (5).to_bytes(8, "big") + b"\x0a",
            (5).to_bytes(8, "big") + bytes(4) + b"\x0d", (5).to_bytes(8, "big") + bytes(4) + b"\x01\x0e",
            (6).to_bytes(8, "big") + b"\x09"],
    }
    for cmpr, pool in pools.items():
        for a in pool:
            for b in pool:
                assert suffix_compare(cmpr, a, b) == U.suffix_cmp(cmpr, a, b), (cmpr, a, b)
    # equal and not byte-equal; and the marks that the point comparers ignore are not ignored here
    assert suffix_compare(T, b"@5", b"@05") == 0
    assert suffix_compare(T, b"@5", b"@5_synthetic") == -1 and suffix_compare(T, b"@5_synthetic", b"@5") == 1
    assert suffix_compare(C, pools[C][2], pools[C][3]) == 0
    assert suffix_compare(C, pools[C][4], pools[C][5]) != 0
    assert suffix_compare(T, b"@7", b"@6") == -1  # newer first: @7 <= @6 < @5


# ---- 2. the Python statement against the reference's data ----------------------------------------------
def test_statement_coalesce_fixture():
    for c in G["coalesce"]:
        _, _, keys = U.parse_span(c["in"])
        _, _, out = U.parse_span(c["out"])
        assert U.coalesce(keys, T) == U.sets_of(out), c


def test_statement_iter_fixture():
    for c in G["iter"]:
        spans = [U.parse_span(x) for x in c["define"]]
        snap = MAX if c["snapshot"] is None else c["snapshot"]
        exp = [(s, e, U.sets_of(ks)) for s, e, ks in map(U.parse_span, c["walk"])]
        assert U.expected_spans([spans], T, snap, defrag=False) == [x for x in exp if x[2]], c
    # the visible-seq-num=10 block under the defragmenter: c-d and d-f hold the same set
    spans = [U.parse_span(x) for x in G["iter"][1]["define"]]
    assert [(s, e) for s, e, _ in U.expected_spans([spans], T, 10)] == [(b"a", b"c"), (b"c", b"f")]


def test_statement_defragmenting_fixture():
    for c in G["defragmenting_iter"]:
        spans = [U.parse_span(x) for x in c["define"]]
        assert U.expected_spans([spans], T) == [U.parse_span(x) for x in c["forward"]], c


def masking_runs(c):
    return [[(s.encode(), e.encode(), [(tr(10 + i, SET), sfx.encode(), v.encode())])]
            for i, (s, e, sfx, v) in enumerate(c["range_keys"])]


def test_statement_masking_fixture():
    for c in G["masking"]:
        runs = masking_runs(c)
        got = [p for p in c["points"] if U.expected_masked(runs, p.encode(), T, c["mask_suffix"].encode())]
        assert sorted(got) == sorted(c["masked"]), c


SKIP_POINT = ([[(b"e", b"m", [(tr(3), b"@9", b"")])], [(b"h", b"q", [(tr(2), b"@6", b"")])],
               [(b"f", b"l", [(tr(1), b"@3", b"")])]], [b"b@2", b"h@5", b"l@8", b"n@4"], b"@7")


def test_statement_skip_point_example():
    """SkipPoint's comment (range_keys.go:300-340): exactly h@5 and n@4 are masked."""
    runs, pts, t = SKIP_POINT
    assert [p for p in pts if U.expected_masked(runs, p, T, t)] == [b"h@5", b"n@4"]


# ---- 3. the set builder ------------------------------------------------------------------------------------
def fixture_runs():
    """(name, runs, snapshot): each fixture case as one run, and the multi-span ones as one run per span."""
    out = []
    for i, c in enumerate(G["coalesce"]):
        out.append(("coalesce %d" % i, [[U.parse_span(c["in"])]], MAX))
    for name in ("iter", "defragmenting_iter"):
        for i, c in enumerate(G[name]):
            spans = [U.parse_span(x) for x in c["define"]]
            snap = c.get("snapshot") or MAX
            out.append(("%s %d" % (name, i), [spans], snap))
            out.append(("%s %d, a run per span" % (name, i), [[s] for s in spans], snap))
    return out


@pytest.mark.parametrize("name,runs,snapshot", fixture_runs(), ids=[c[0] for c in fixture_runs()])
def test_set_fixtures(name, runs, snapshot):
    check_set(runs, T, snapshot, name)


@pytest.mark.parametrize("name,runs,comparer,snapshots", CASES, ids=[c[0] for c in CASES])
def test_set_cases(name, runs, comparer, snapshots):
    for s in snapshots:
        exp, got = check_set(runs, comparer, s, name)
        assert got["status_mask"] == 0
        if name in ("no runs", "an empty run", "only unset and del"):
            assert got["n_kv"] == 0
        if name == "chain of 300" or name == "chain of 300 over 2 runs":
            assert [(a, b) for a, b, _ in exp] == [(U.gen_key(0), U.gen_key(300))]
        if name.startswith("chain with one other value"):
            assert [(a, b) for a, b, _ in exp] == [(U.gen_key(0), U.gen_key(150)), (U.gen_key(150), U.gen_key(151)),
                                                   (U.gen_key(151), U.gen_key(300))]
        if name == "chain broken by an empty interval" and s == MAX:
            assert [(a, b) for a, b, _ in exp] == [(U.gen_key(0), U.gen_key(20)), (U.gen_key(21), U.gen_key(40))]
        if name == "equal suffixes, other bytes":
            assert exp == [(U.gen_key(0), U.gen_key(6), [(tr(100), b"@7", b"v")])]  # the leftmost's bytes
        if name == "crdb equal suffixes, other bytes":
            assert len(exp) == 1 and exp[0][2][0][1].endswith(b"\x0a")
        if name in ("synthetic mark is another suffix", "crdb synthetic bit is another suffix") and s == MAX:
            assert len(exp) == 6
        if name.endswith("candidates"):
            assert len(exp) == 1 and len(exp[0][2]) > 1


def test_set_same_sequence_rules():
    one = lambda keys, snap=MAX: [k for _, _, ks in U.expected_spans([[(b"a", b"b", keys)]], T, snap) for k in ks]  # noqa: E731
    S, Un, X = (lambda q, s, v: (tr(q), s, v)), (lambda q, s: (tr(q, UNSET), s, b"")), (lambda q: (tr(q, DEL), b"", b""))
    assert one([S(5, b"@3", b"v"), Un(5, b"@3")]) == [S(5, b"@3", b"v")]
    keys = [S(10, b"@5", b"x"), Un(10, b"@4"), X(10), S(9, b"@4", b"y"), S(4, b"@3", b"z")]
    assert one(keys) == [S(10, b"@5", b"x")]           # the DEL spares its own sequence number and cuts all below
    assert one(keys, 10) == [S(9, b"@4", b"y"), S(4, b"@3", b"z")]  # at the snapshot: invisible, cuts nothing
    assert one([S(9, b"@4", b"y")], 9) == []


def test_set_statuses():
    good = [(b"a", b"b", [(tr(5), b"@1", b"v")]), (b"c", b"d", [(tr(5), b"@1", b"v")])]
    rangedel = [(b"a", b"b", [(5 << 8 | 15, b"", b"")])]
    unsorted = [good[1], good[0]]
    overlap = [(b"a", b"c", good[0][2]), (b"b", b"d", good[0][2])]
    same_start = [(b"a", b"c", good[0][2]), (b"a", b"d", good[0][2])]
    Un, A = N.PBL_UNSUPPORTED, N.PBL_INVALID_ARG
    for runs, st in (([rangedel, good], Un), ([good, overlap], A), ([unsorted, rangedel], Un), ([[], good, []], 0)):
        hosts = [U.run_host(r) for r in runs]
        got = build_set_host(hosts, T)
        if st:
            assert_same(got, U.empty_set(st), st)
        assert got["blk_status"].tolist() == [st]
        cov, mst = mask_host(hosts, point_batch([b"a@0", b"b@0"]), T, b"@9")
        assert mst == st and (st == 0 or cov.tolist() == [0, 0])
    # (the Python writer joins abutting spans by bytes, so unsorted / same_start runs are written as raw KVs)
    for kvs in (unsorted, same_start):
        h = U.layout([kvs])
        assert build_set_host([h], T)["blk_status"].tolist() == [A]
    bad = U.run_host(good)
    bad["blk_status"] = np.array([N.PBL_CORRUPT_BOUNDS], np.uint32)
    assert build_set_host([U.run_host(rangedel), bad], T)["blk_status"].tolist() == [N.PBL_CORRUPT_BOUNDS]
    short = U.run_host(good)
    short["n_kv"] = 1
    assert build_set_host([short], T)["blk_status"].tolist() == [A]


def test_argument_errors():
    run = U.run_host([(b"a", b"b", [(tr(5), b"@1", b"v")])])
    with pytest.raises(DecodeError, match="INVALID_ARG"):
        build_set_host([run] * 17, T)
    with pytest.raises(DecodeError, match="INVALID_ARG"):
        build_set_host([run], 3)
    with pytest.raises(DecodeError, match="INVALID_ARG"):
        mask_host([run] * 17, point_batch([b"a@1"]), T, b"@9")
    assert build_set_host([run] * 16, T)["n_kv"] == 1
    lib = N.lib()
    assert lib.pbl_rangekey_set_host(None, None, None) == N.PBL_INVALID_ARG
    assert lib.pbl_rangekey_mask(None, None, None, 0, 0, 0, None, 0, None, None) == N.PBL_INVALID_ARG
    assert lib.pbl_rangekey_clip_host(None, None, None, None, None) == N.PBL_INVALID_ARG


def test_overflow_on_each_output():
    runs = [U.chain(5, value_of=lambda i: b"value%d" % i, suffix_of=lambda i: b"@%d" % i, keys=2)]
    hosts = [U.run_host(r) for r in runs]
    full = build_set_host(hosts, T)
    n, kb, vb = full["n_kv"], full["key_bytes_total"], full["val_bytes_total"]
    sb, xb = int(full["blk_suffix_base"][1]), int(full["blk_value_base"][1])
    assert n == 10 and min(kb, vb, sb, xb) > 0
    for cap, ecap in ((Capacity(n - 1, kb, vb, 0), (sb, xb)), (Capacity(n, kb - 1, vb, 0), (sb, xb)),
                      (Capacity(n, kb, vb - 1, 0), (sb, xb)), (Capacity(n, kb, vb, 0), (sb - 1, xb)),
                      (Capacity(n, kb, vb, 0), (sb, xb - 1))):
        got = build_set_host(hosts, T, cap=cap, extra_cap=ecap)
        assert_same(got, sized(full), (cap, ecap))
    assert_same(build_set_host(hosts, T, cap=Capacity(n, kb, vb, 0), extra_cap=(sb, xb)), full)


# ---- 4. clip --------------------------------------------------------------------------------------------------
CLIP_RUNS = [[(b"b", b"f", [(tr(9), b"@5", b"x"), (tr(8), b"@3", b"y")]), (b"f", b"h", [(tr(9), b"@5", b"z")]),
              (b"m", b"p", [(tr(9), b"@1", b"w")])]]
CLIP_RANGES = [(b"c", b"e"), (b"b", b"f"), (b"f", b"h"), (b"h", b"m"), (b"i", b"k"), (None, None), (None, b"c"), (b"n", None),
               (b"a", b"z"), (b"e", b"n"), (b"p", None), (None, b"b"), (b"", b"bb")]


@pytest.mark.parametrize("n", [0, 1, len(CLIP_RANGES), 65])
def test_clip(n):
    set_ = host_set(CLIP_RUNS, T)
    spans = U.expected_spans(CLIP_RUNS, T)
    ranges = [CLIP_RANGES[i % len(CLIP_RANGES)] for i in range(n)]
    got = clip_host(set_, [r[0] for r in ranges], [r[1] for r in ranges], T)
    exp = [U.clip_spans(spans, lo, up, T) for lo, up in ranges]
    assert_same(got, U.layout(exp), n)
    if n == len(CLIP_RANGES):
        assert [len(x) for x in exp] == [1, 1, 1, 0, 0, 3, 1, 1, 3, 3, 0, 0, 1]
        assert exp[0] == [(b"c", b"e", spans[0][2])]          # strictly inside one span
        assert U.spans_of_host(got, 9) == [(b"e", b"f", spans[0][2]), (b"f", b"h", spans[1][2]), (b"m", b"n", spans[2][2])]


def test_clip_of_a_set_with_a_status_and_overflow():
    bad = build_set_host([U.run_host([(b"a", b"b", [(5 << 8 | 15, b"", b"")])])], T)
    got = clip_host(bad, [b"a", None], [b"b", None], T)
    assert_same(got, U.layout([[], []], [N.PBL_UNSUPPORTED] * 2))
    set_ = host_set(CLIP_RUNS, T)
    full = clip_host(set_, [None], [None], T)
    got = clip_host(set_, [None], [None], T, cap=Capacity(full["n_kv"] - 1, 100, 100, 0), extra_cap=(100, 100))
    assert_same(got, sized(full))


# ---- 5. the mask ----------------------------------------------------------------------------------------------
def check_mask(runs, comparer, keys, t, snapshot=MAX, cover=None, ctx=""):
    hosts = [U.run_host(r) for r in runs]
    batch = point_batch(keys)
    exp = U.expected_cover(runs, keys, comparer, t, snapshot, cover)
    got, st = mask_host(hosts, batch, comparer, t, snapshot, cover)
    assert st == 0 and got.tolist() == exp, (ctx, "runs")
    set_ = build_set_host(hosts, comparer, snapshot)
    assert mask_set_host(set_, batch, comparer, t, cover).tolist() == exp, (ctx, "set")
    return exp


def test_mask_fixtures():
    for c in G["masking"]:
        keys = sorted(p.encode() for p in c["points"])
        exp = check_mask(masking_runs(c), T, keys, c["mask_suffix"].encode(), ctx=c["mask_suffix"])
        assert sorted(k for k, m in zip(keys, exp) if m) == sorted(p.encode() for p in c["masked"])
    runs, pts, t = SKIP_POINT
    assert check_mask(runs, T, pts, t) == [0, ALL, 0, ALL]


def test_mask_edges():
    runs = [[(b"c", b"f", [(tr(9), b"", b"nosuffix"), (tr(8), b"@6", b"x"), (tr(7), b"@3", b"y")]),
             (b"h", b"k", [(tr(9), b"", b"only")])]]
    keys = [b"b@1", b"c", b"c@1", b"c@5", b"c@6", b"c@7", b"e@2", b"f@1", b"g@1", b"h@1", b"j@0"]
    # a key equal to a start is covered, one equal to an end is not; a point without a suffix; an
    # empty-suffix range key never masks
    assert check_mask(runs, T, keys, b"@9") == [0, 0, ALL, ALL, 0, 0, ALL, 0, 0, 0, 0]
    assert check_mask(runs, T, keys, b"@5") == [0, 0, ALL, 0, 0, 0, ALL, 0, 0, 0, 0]   # @6 is below the threshold
    assert check_mask(runs, T, keys, b"@2") == [0] * len(keys)                            # t above every suffix
    assert check_mask(runs, T, keys, b"") == [0, 0, ALL, ALL, 0, 0, ALL, 0, 0, 0, 0]     # the empty threshold
    # a cover that is passed in is kept where nothing is masked
    cover = [5, 0, 7, 0, 9, 0, 0, 11, 0, 0, 13]
    assert check_mask(runs, T, keys, b"@9", cover=cover) == [5, 0, ALL, ALL, 9, 0, ALL, 11, 0, 0, 13]


def test_mask_bad_block_and_sizes():
    runs = [U.chain(4, suffix_of=lambda i: b"@%d" % (5 + i))]
    hosts = [U.run_host(r) for r in runs]
    keys = [U.gen_key(i % 5) + b"@%d" % (i % 9) for i in range(65)]
    blocks = [[(k, 7 << 8 | 1, b"v") for k in keys[:30]], None, [(k, 7 << 8 | 1, b"v") for k in keys[30:]]]
    batch = host_from_blocks(blocks)
    exp = U.expected_cover(runs, keys, T, b"@9")
    got, _ = mask_host(hosts, batch, T, b"@9")
    assert got.tolist() == exp and 0 < sum(1 for x in exp if x) < 65
    assert mask_set_host(build_set_host(hosts, T), batch, T, b"@9").tolist() == exp


@pytest.mark.parametrize("name,runs,comparer,snapshots", CASES, ids=[c[0] for c in CASES])
def test_mask_cases(name, runs, comparer, snapshots):
    keys = U.points_for(runs, comparer)
    if len(keys) > 400:
        keys = random.Random(1).sample(keys, 400)
        keys.sort(key=functools.cmp_to_key(lambda a, b: U.key_compare(comparer, a, b)))
    t = {T: b"@30", C: (20).to_bytes(8, "big") + b"\x09", D: b"s"}[comparer]
    for s in snapshots:
        check_mask(runs, comparer, keys, t, s, ctx=(name, s))


# ---- 6. the ABI ---------------------------------------------------------------------------------------------
def test_struct_layout():
    buf = (ctypes.c_uint64 * 16)()
    n = N.lib().pbl_rangekey_struct_layout(buf, 16)
    S = N.RangekeyRunsC
    assert list(buf[:n]) == [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
