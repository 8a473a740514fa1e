"""Range deletions in the read path without a GPU: the ABI
additions, the host set builder and the host cover against the Python statement
of the rule (rangedelutil: brute force over unfragmented tombstones), the view's
host form with a cover, and the reference's own testdata/range_del replayed
through merge -> cover -> view (tests/golden/range_del.json)."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from mergeutil import BAD, C, D, T, crdb_key
from pebble_amd import _native as N
from pebble_amd.batch import Capacity
from pebble_amd.merge import merge_host
from pebble_amd.rangedel import build_set_host, cover_host
from pebble_amd.rowblk import Writer, make_trailer
from pebble_amd.visible import visible_host
from rangedelutil import (RANGEDEL, assert_visible_rd_is, brute_cover, expected_cover, expected_set, expected_visible_rd,
                          fragment, golden_sections, load_golden, section_levels, random_runs, replay_case, run_block, run_host, run_kvs,
                          set_kvs)
from scanutil import result_kvs
from visibleutil import MAX, MERGE, SET, assert_same, cases, host_from_blocks, tr

G = load_golden()
U, A, O = N.PBL_UNSUPPORTED, N.PBL_INVALID_ARG, N.PBL_OVERFLOW


def rd(start, end, seq):
    return (start, make_trailer(seq, RANGEDEL), end)


def test_struct_layout_and_abi():
    L = N.lib()
    buf = (ctypes.c_uint64 * 16)()
    n = L.pbl_rangedel_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 16)
    S = N.RangedelRunsC
    assert list(buf[:n]) == [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_] and n == 7
    assert L.pbl_abi_version() == 9
    # the other lists are what they were
    assert L.pbl_visible_struct_layout(None, 0) == 10 and L.pbl_merge_struct_layout(None, 0) == 11
    prev = 0
    for t in (0, 1, 127, 128, 129, 1 << 20):
        w = int(L.pbl_rangedel_workspace_bytes(t))
        assert w % 16 == 0 and w >= prev and w >= 32 * t
        prev = w


def test_invalid_arguments_return_before_any_device_call():
    L = N.lib()
    arr = np.zeros(64, np.uint64)
    p = arr.ctypes.data

    def struct(skip=()):
        d = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base",
                  "blk_val_base", "blk_status", "totals"):
            if f not in skip:
                setattr(d, f, p)
        d.kv_cap = d.key_cap = 8
        return d

    def runs(n=1, comparer=D, skip=(), n_kv=True, count=0):
        a = (N.DecodeOutC * 17)(*[struct(skip) for _ in range(17)])
        c = (ctypes.c_uint64 * 17)(*([count] * 17))
        return (a, c), N.RangedelRunsC(ctypes.cast(a, ctypes.POINTER(N.DecodeOutC)),
                                       ctypes.cast(c, ctypes.POINTER(ctypes.c_uint64)) if n_kv else None, n, comparer, MAX)

    ws = np.zeros(4096 + 16, np.uint8)
    wp = (ws.ctypes.data + 15) // 16 * 16
    out = struct()

    def both(rs, o=out, ok=False):
        got = [L.pbl_rangedel_set(ctypes.byref(rs) if rs else None, ctypes.byref(o) if o else None, ctypes.c_void_p(wp),
                                  4096, None) if not ok else N.PBL_OK,
               L.pbl_rangedel_set_host(ctypes.byref(rs) if rs else None, ctypes.byref(o) if o else None)]
        return got

    assert both(None) == [A, A]
    k, rs = runs()
    assert both(rs, None) == [A, A]
    for kw in (dict(n=17), dict(comparer=C + 1), dict(n_kv=False), dict(count=1 << 31)):
        k, rs = runs(**kw)
        assert both(rs) == [A, A], kw
    for f in ("trailer", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base", "blk_val_base",
              "blk_status"):
        k, rs = runs(skip=(f,))
        assert both(rs) == [A, A], f
    for f in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_status", "totals", "trailer", "key_off", "key_bytes"):
        k, rs = runs()
        assert both(rs, struct((f,))) == [A, A], f
    # the workspace: NULL, misaligned, one byte short
    k, rs = runs(count=3)
    need = int(L.pbl_rangedel_workspace_bytes(3))
    assert L.pbl_rangedel_set(ctypes.byref(rs), ctypes.byref(out), None, 4096, None) == A
    assert L.pbl_rangedel_set(ctypes.byref(rs), ctypes.byref(out), ctypes.c_void_p(wp + 8), 4096, None) == A
    assert L.pbl_rangedel_set(ctypes.byref(rs), ctypes.byref(out), ctypes.c_void_p(wp), need - 1, None) == A
    # the cover
    s, b = struct(), struct()
    cv = lambda s_, b_, c_=D, o_=p: L.pbl_rangedel_cover(ctypes.byref(s_) if s_ else None, ctypes.byref(b_) if b_ else None,  # noqa: E731
                                                           1, 4, c_, o_, None)
    assert cv(None, b) == A and cv(s, None) == A and cv(s, b, C + 1) == A and cv(s, b, D, None) == A
    assert cv(struct(("trailer",)), b) == A and cv(s, struct(("key_off",))) == A
    k, rs = runs()
    assert L.pbl_rangedel_cover_host(None, ctypes.byref(b), 1, p, None) == A
    assert L.pbl_rangedel_cover_host(ctypes.byref(rs), None, 1, p, None) == A
    assert L.pbl_rangedel_cover_host(ctypes.byref(rs), ctypes.byref(b), 1, None, None) == A
    assert not arr.any() and not ws.any()


def test_python_fragmenter_matches_the_reference_builds():
    kinds = G["kinds"]
    assert len(G["fragments"]) == 3

    def parse(spans):
        out = []
        for s in spans:
            keys = []
            for k in s["keys"]:
                w = k.split(",")
                keys.append((int(w[0][1:]), kinds[w[1]], k))
            out.append((s["start"].encode(), s["end"].encode(), keys))
        return out

    for b in G["fragments"]:
        got = fragment(parse(b["input"]))
        assert [(s, e, [k[2] for k in ks]) for s, e, ks in got] == \
            [(s, e, [k[2] for k in ks]) for s, e, ks in parse(b["output"])]
    # and the run form: overlapping tombstones become a valid run
    kvs = run_kvs([(b"a", b"d", 11), (b"b", b"e", 12)])
    assert [(s, t >> 8, e) for s, t, e in kvs] == [(b"a", 11, b"b"), (b"b", 12, b"d"), (b"b", 11, b"d"), (b"d", 12, b"e")]


SHAPES = [(D, 1, 1, "distinct"), (D, 3, 40, "distinct"), (D, 16, 65, "distinct"), (D, 4, 30, "same_start"),
          (D, 16, 9, "shared"), (D, 5, 1, "shared"), (T, 3, 20, "distinct"), (T, 4, 7, "shared"), (C, 3, 20, "distinct"),
          (C, 4, 7, "shared")]


@pytest.mark.parametrize("comparer,n_runs,per_run,shape", SHAPES, ids=["%d-%dx%d-%s" % s for s in SHAPES])
def test_host_set_and_cover_equal_the_python_model(comparer, n_runs, per_run, shape):
    rng = random.Random(7 * n_runs + per_run)
    runs = random_runs(rng, n_runs, per_run, comparer, shape=shape)
    hosts = [run_host(kvs) for kvs in runs]
    # the points: every boundary, as a batch of two blocks
    keys = [k for k, _ in expected_set(runs, comparer)]
    blocks = [[(k, tr(500), b"v") for k in keys[::2]], [(k, tr(500), b"") for k in keys[1::2]]]
    batch = host_from_blocks(blocks)
    for snapshot in (MAX, 500, 1):
        r = build_set_host(hosts, comparer, snapshot)
        assert r["status_mask"] == 0 and set_kvs(r) == expected_set(runs, comparer, snapshot), (shape, snapshot)
        assert set_kvs(r)[-1][1] == 0
        cov, st = cover_host(hosts, batch, comparer, snapshot)
        assert st == 0 and cov.tolist() == expected_cover(runs, batch, comparer, snapshot).tolist()
    if shape == "shared":
        assert len(keys) < 2 * n_runs * per_run
    if shape == "distinct":
        assert len(keys) == 2 * n_runs * per_run


def decode_host(blocks):
    """Row blocks through the CPU oracle, in to_host()'s layout."""
    off, buf = [], bytearray()
    for b in blocks:
        off.append(len(buf))
        buf += b + bytes(-len(b) % 8)
    r = oracle.decode_batch(np.frombuffer(bytes(buf) + bytes(16), np.uint8), np.array(off, np.uint64),
                            np.array([len(b) for b in blocks], np.uint32))
    r["n_slow_blocks"] = 0
    return r


def row_block(kvs, restart=4):
    w = Writer(restart)
    for k, t, v in kvs:
        w.add(k, t, v)
    return w.finish()


def golden_hosts(define):
    secs = golden_sections(define, G["kinds"])
    points = [decode_host([row_block(pts)]) for pts, _, _ in secs]
    runs = [decode_host([run_block(kvs)]) for _, kvs, _ in secs]
    tombs = [t for _, _, ts in secs for t in ts]
    return points, runs, tombs


def test_golden_counts():
    """What the parametrised replay below goes through: every kept define and case."""
    assert G["n_defines"] == len(G["defines"]) == 8
    assert sum(len(d["cases"]) for d in G["defines"]) == G["n_cases"] == 60
    assert sum(len(c["expected"]) for d in G["defines"] for c in d["cases"]) == G["n_lines"] == 308


@pytest.mark.parametrize("di", range(len(G["defines"])))
def test_golden_range_del_cases(di):
    """Every kept case of testdata/range_del, define by define: each section one
    point block and one run (rowblk.Writer), merged, covered, viewed, replayed.
    The sections' levels go in (rangedelutil.section_levels): define 3
    ("Overlapping range deletions in different memtables") holds the tombstone
    c#13 in a newer memtable than the point c#14, which the reference deletes
    level by level and the sequence numbers alone would keep."""
    d = G["defines"][di]
    points, runs, tombs = golden_hosts(d)
    lv = section_levels(d)
    leveled = [(s, e, t, lv[i]) for i, (_, _, ts) in enumerate(golden_sections(d, G["kinds"])) for s, e, t in ts]
    assert all(p["status_mask"] == 0 for p in points + runs), di
    merged, src_run, _ = merge_host(points, comparer=D)
    wrong = []
    for c in d["cases"]:
        cov, st = cover_host(runs, merged, D, c["seq"], levels=lv, src_run=src_run, run_levels=lv)
        assert st == 0
        # the third statement: brute force over the unfragmented tombstones
        assert cov.tolist() == [brute_cover(leveled, k, D, c["seq"], lv[int(src_run[j])])
                                for j, (k, _, _, _) in enumerate(result_kvs(merged, 0))]
        r = visible_host(merged, comparer=D, snapshot=c["seq"], cover=cov)[0]
        assert r["status_mask"] == 0
        kvs = [(k, v) for k, _, v, _ in result_kvs(r, 0)]
        got = replay_case(kvs, c)
        wrong += [(c["op"], c["seq"], i, g, e) for i, (g, e) in enumerate(zip(got, c["expected"])) if g != e]
        assert len(got) == len(c["expected"])
        if di != 3:  # sequence numbers ordered by level: the sequence-number rule alone gives the same cover
            plain, _ = cover_host(runs, merged, D, c["seq"])
            seqs = merged["trailer"] >> 8
            assert ((plain > seqs) == (cov > seqs)).all(), (di, c["seq"])
    print("define", di, len(d["cases"]), "cases,", len(wrong), "lines differ", wrong)
    assert not wrong, (di, wrong)


def test_levels_matter_only_where_sequence_numbers_are_not_ordered_by_level():
    """Define 3 without levels: the sequence-number rule keeps c#14 under c#13."""
    d = G["defines"][3]
    points, runs, _ = golden_hosts(d)
    lv = section_levels(d)
    assert lv == [3, 2, 1, 0]
    merged, src_run, _ = merge_host(points, comparer=D)
    at = next(j for j, (k, t, _, _) in enumerate(result_kvs(merged, 0)) if (k, t >> 8) == (b"c", 14))
    plain, _ = cover_host(runs, merged, D, 16)
    leveled, _ = cover_host(runs, merged, D, 16, levels=lv, src_run=src_run, run_levels=lv)
    assert plain[at] == 13 and leveled[at] == N.PBL_RANGEDEL_ALL
    # the set records the shallowest covering level per boundary
    s = build_set_host(runs, D, 16, levels=lv)
    assert [(k, c, int(e)) for (k, c), e in zip(set_kvs(s), s["entry_off"])] == [(b"a", 11, 3), (b"b", 13, 2), (b"c", 13, 1), (b"d", 0, 0)]
    assert build_set_host(runs, D, 16)["entry_off"] is None
    assert section_levels({"sections": [{"level": x} for x in ("L0", "L0", "L1", "L1", "mem", "L3")]}) == [2, 1, 3, 3, 0, 4]


def test_without_the_cover_the_first_define_is_wrong():
    """The behavioural difference: get seq=16 of b returns bcd without the cover."""
    d = G["defines"][0]
    points, runs, _ = golden_hosts(d)
    merged = merge_host(points, comparer=D)[0]
    c = next(c for c in d["cases"] if c["op"] == "get" and c["seq"] == 16)
    assert "b: pebble: not found" in c["expected"]
    plain = dict((k, v) for k, _, v, _ in result_kvs(visible_host(merged, comparer=D, snapshot=16)[0], 0))
    assert plain[b"b"] == b"bcd"
    cov, _ = cover_host(runs, merged, D, 16)
    with_rd = dict((k, v) for k, _, v, _ in result_kvs(visible_host(merged, comparer=D, snapshot=16, cover=cov)[0], 0))
    assert b"b" not in with_rd and with_rd[b"a"] == b"d"


def view(points, runs, comparer=D, snapshot=MAX, keep=False):
    h = host_from_blocks([points])
    cov, st = cover_host([run_host(r) for r in runs], h, comparer, snapshot)
    assert st == 0
    res = visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep, cover=cov)
    assert_visible_rd_is(res, expected_visible_rd(h, comparer, snapshot, keep, cov))
    return [(k, t >> 8, v) for k, t, v, _ in result_kvs(res[0], 0)], cov.tolist()


def test_edges_of_the_rule():
    # s == t survives (the last define of testdata/range_del), s < t does not
    pts = [(b"a", tr(11, MERGE), b"1"), (b"a", tr(10), b"2"), (b"b", tr(11), b"x"), (b"b", tr(12), b"y")]
    pts.sort(key=lambda kv: (kv[0], -kv[1]))
    got, cov = view(pts, [[rd(b"a", b"d", 11)]])
    assert got == [(b"a", 11, b"1"), (b"b", 12, b"y")] and cov == [11, 11, 11, 11]
    # the start key is inclusive, the end key exclusive
    pts = [(k, tr(5), k) for k in (b"a", b"b", b"b\x00", b"c", b"c\x00")]
    got, cov = view(pts, [[rd(b"b", b"c", 9)]])
    assert [k for k, _, _ in got] == [b"a", b"c", b"c\x00"] and cov == [0, 9, 9, 0, 0]
    # a tombstone at or above the snapshot is ignored, a lower one at the same span still applies
    run = [rd(b"a", b"z", 20), rd(b"a", b"z", 10)]
    pts = [(b"k", tr(15), b"new"), (b"k", tr(5), b"old")]
    assert view(pts, [run], snapshot=MAX) == ([], [20, 20])
    assert view(pts, [run], snapshot=21) == ([], [20, 20])
    assert view(pts, [run], snapshot=20) == ([(b"k", 15, b"new")], [10, 10])
    assert view(pts, [run], snapshot=11) == ([], [10, 10])       # (15 is above the snapshot, 5 is deleted)
    assert view(pts, [run], snapshot=10) == ([(b"k", 5, b"old")], [0, 0])
    # the same two tombstones in two runs
    assert view(pts, [[run[0]], [run[1]]], snapshot=20) == ([(b"k", 15, b"new")], [10, 10])
    # a deleted SET inside a MERGE chain does not end it
    pts2 = [(b"m", tr(30, MERGE), b"c"), (b"m", tr(25, MERGE), b"b"), (b"m", tr(8, SET), b"deleted"), (b"m", tr(4, SET), b"x")]
    assert view(pts2, [[rd(b"a", b"z", 9)]]) == ([(b"m", 30, b"bc")], [9, 9, 9, 9])
    assert view(pts2, [[rd(b"a", b"z", 9)]], keep=True)[0] == [(b"m", 30, b"c"), (b"m", 25, b"b")]
    assert view(pts2, [[rd(b"a", b"z", 5)]]) == ([(b"m", 30, b"deletedbc")], [5, 5, 5, 5])
    # a deleted head: the next visible version heads the group
    assert view(pts2, [[rd(b"a", b"z", 26)]]) == ([(b"m", 30, b"c")], [26] * 4)
    assert view(pts2, [[rd(b"a", b"z", 31)]]) == ([], [31] * 4)
    pts3 = [(b"m", tr(30, SET), b"new"), (b"m", tr(3, SET), b"old")]
    assert view(pts3, [[rd(b"m", b"n", 4)]]) == ([(b"m", 30, b"new")], [4, 4])


def test_comparer_boundaries():
    # TESTKEYS: a@5 sorts after a@9; a tombstone [a@9, b) covers a@5 but not the bare prefix a
    pts = [(b"a", tr(1), b"bare"), (b"a@9", tr(1), b"9"), (b"a@5", tr(1), b"5"), (b"a@5_synthetic", tr(2), b"5s"), (b"b", tr(1), b"b")]
    got, cov = view([pts[0], pts[1], pts[3], pts[2], pts[4]], [[rd(b"a@9", b"b", 7)]], comparer=T)
    assert got == [(b"a", 1, b"bare"), (b"b", 1, b"b")] and cov == [0, 7, 7, 7, 0]
    # boundaries without suffixes cover every version of the prefix
    got, cov = view([pts[0], pts[1], pts[3], pts[2], pts[4]], [[rd(b"a", b"a@5", 7)]], comparer=T)
    assert [k for k, _, _ in got] == [b"a@5_synthetic", b"b"] and cov == [7, 7, 0, 0, 0]
    # equal boundaries with different bytes are one boundary: the first's bytes
    r = build_set_host([run_host([rd(b"a@5_synthetic", b"c", 3)]), run_host([rd(b"a", b"a@5", 4)])], T)
    assert set_kvs(r) == [(b"a", 4), (b"a@5_synthetic", 3), (b"c", 0)]
    # CRDB: bare roachkey first, then versions descending
    k = lambda w=None, lg=None: crdb_key(b"k1", w, lg)  # noqa: E731
    pts = [(k(), tr(1), b"bare"), (k(9), tr(1), b"9"), (k(5, 0), tr(1), b"5"), (crdb_key(b"k2"), tr(1), b"k2")]
    got, cov = view(pts, [[rd(k(9), crdb_key(b"k2"), 7)]], comparer=C)
    assert [v for _, _, v in got] == [b"bare", b"k2"] and cov == [0, 7, 7, 0]
    got, cov = view(pts, [[rd(k(), k(5), 7)]], comparer=C)  # the end k1@5 equals k1@5,0 under the comparer
    assert [v for _, _, v in got] == [b"5", b"k2"] and cov == [7, 7, 0, 0]
    r = build_set_host([run_host([rd(k(5, 0), crdb_key(b"k3"), 3)]), run_host([rd(k(), k(5), 4)])], C)
    assert set_kvs(r) == [(k(), 4), (k(5, 0), 3), (crdb_key(b"k3"), 0)]


def test_empty_runs_and_no_runs():
    batch = host_from_blocks([[(b"a", tr(1), b"")], []])
    for hosts in ([], [run_host([])], [run_host([]), run_host([rd(b"a", b"b", 3)]), run_host([])]):
        r = build_set_host(hosts, D)
        assert r["status_mask"] == 0 and r["blk_status"].tolist() == [0]
        assert set_kvs(r) == ([(b"a", 3), (b"b", 0)] if len(hosts) == 3 else [])
        cov, st = cover_host(hosts, batch, D)
        assert st == 0 and cov.tolist() == [3 if len(hosts) == 3 else 0]


def test_statuses_and_their_precedence():
    good = [rd(b"a", b"b", 5), rd(b"c", b"d", 5)]
    bad_status = host_from_blocks([None])
    other = run_host(good)
    other["blk_status"] = np.array([N.PBL_CORRUPT_BOUNDS], np.uint32)
    kind = [(b"a", make_trailer(5, SET), b"b")]
    invalid_key = run_host(good)
    invalid_key["kv_flags"] = np.array([0, N.PBL_KV_INVALID_KEY], np.uint8)
    unsorted = [rd(b"c", b"d", 5), rd(b"a", b"b", 5)]
    ascending = [rd(b"a", b"b", 5), rd(b"a", b"b", 6)]
    empty_span = [rd(b"a", b"a", 5)]
    inverted = [rd(b"b", b"a", 5)]
    overlap = [rd(b"a", b"c", 5), rd(b"b", b"d", 5)]
    same_start_other_end = [rd(b"a", b"c", 6), rd(b"a", b"d", 5)]
    count = run_host(good)
    count["n_kv"] = 1  # announces fewer KVs than it holds
    batch = host_from_blocks([[(b"a", tr(1), b"")]])

    def status(hosts):
        hosts = [h if isinstance(h, dict) else run_host(h) for h in hosts]
        r = build_set_host(hosts, D)
        st = int(r["blk_status"][0])
        assert (st == 0 or (r["n_kv"] == 0 and r["key_bytes_total"] == 0)) and r["n_bad_blocks"] == (1 if st else 0)
        assert r["status_mask"] == ((1 << st) if st else 0)
        cov, st2 = cover_host(hosts, batch, D)
        assert st2 == st and (st == 0 or not cov.any())
        return st

    assert status([good, bad_status]) == BAD
    assert status([good, other, bad_status]) == N.PBL_CORRUPT_BOUNDS  # the first in run order
    assert status([kind]) == U and status([good, invalid_key]) == U
    assert status([good, empty_span]) == 0  # an empty fragment covers nothing (the golden h tables hold [a, a))
    for run in (unsorted, ascending, inverted, overlap, same_start_other_end, count):
        assert status([good, run]) == A, run
    # precedence: a run's status, then the kind, then the fragmentation
    assert status([unsorted, kind, bad_status]) == BAD
    assert status([unsorted, kind]) == U and status([kind, unsorted]) == U
    assert status([good]) == 0


def test_overflow_writes_sizes_and_nothing_else():
    runs = random_runs(random.Random(3), 3, 10)
    hosts = [run_host(kvs) for kvs in runs]
    full = build_set_host(hosts, D)
    n, kb = full["n_kv"], full["key_bytes_total"]
    assert n == 60 and full["val_bytes_total"] == 0
    exact = build_set_host(hosts, D, cap=Capacity(n, kb, 0, 0))
    assert set_kvs(exact) == set_kvs(full)
    for cap in (Capacity(n - 1, kb, 0, 0), Capacity(n, kb - 1, 0, 0)):
        r = build_set_host(hosts, D, cap=cap)
        assert r["status_mask"] == 1 << O and (r["n_kv"], r["key_bytes_total"]) == (n, kb)
        assert r["blk_kv_base"].tolist() == [0, n] and r["blk_key_base"].tolist() == [0, kb] and r["blk_status"].tolist() == [0]
        assert len(r["trailer"]) == 0 and not r["key_off"].any()


CASES = cases()
PARAMS = [(name, comparer, blocks, s, keep) for name, comparer, blocks, snaps in CASES for s in snaps for keep in (False, True)]
IDS = ["%s-%s%s" % (p[0], "max" if p[3] == MAX else p[3], "-keep" if p[4] else "") for p in PARAMS]


@pytest.mark.parametrize("name,comparer,blocks,snapshot,keep", PARAMS, ids=IDS)
def test_no_cover_equals_the_existing_entry_point_and_a_cover_the_model(name, comparer, blocks, snapshot, keep):
    h = host_from_blocks(blocks)
    plain = visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep)
    zero = visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep, cover=np.zeros(h["n_kv"], np.uint64))
    assert_same(plain, zero, name)
    # NULL through the _rd entry point itself
    L = N.lib()
    from pebble_amd.merge import host_struct
    keep_alive = []
    vin = N.VisibleInC(host_struct(h, keep_alive), len(blocks), comparer, 0, snapshot)
    nb = len(blocks)
    b = {k: np.zeros(nb + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base")}
    st = np.zeros(max(nb, 1), np.uint32)
    tot = N.TotalsC()
    o = N.DecodeOutC()
    for k, v in b.items():
        setattr(o, k, v.ctypes.data)
    o.blk_status = st.ctypes.data
    o.totals = ctypes.addressof(tot)
    vo = N.VisibleOutC(o, None, None)
    assert L.pbl_visible_batch_host_rd(ctypes.byref(vin), ctypes.byref(vo), N.PBL_VISIBLE_KEEP_OPERANDS if keep else 0, None) == 0
    assert (tot.n_kv, tot.key_bytes, tot.val_bytes) == (plain[0]["n_kv"], plain[0]["key_bytes_total"], plain[0]["val_bytes_total"])
    assert st[:nb].tolist() == plain[0]["blk_status"].tolist()
    # a cover drawn at random against the Python model
    rng = random.Random(len(name) + int(keep))
    seqs = sorted({int(t) >> 8 for t in h["trailer"]}) or [1]
    cov = np.array([rng.choice([0, 0, rng.choice(seqs), rng.choice(seqs) + 1]) for _ in range(h["n_kv"])], np.uint64)
    res = visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep, cover=cov)
    assert_visible_rd_is(res, expected_visible_rd(h, comparer, snapshot, keep, cov), name)
