"""Batched k-way merge without a GPU: the ABI additions (pbl_merge_struct_layout,
the workspace size, every invalid-argument return, all before any device call)
and pbl_merge_batch_host -- a plain k-way merge over the same ikey_cmp the
device kernels instantiate -- against Python's `sorted` over pbl_key_compare
(mergeutil.expected_merge) on hand-built runs: the three comparers, run lengths
around the wave and the tile, ties, unsorted and bad blocks, overflow."""
import ctypes

import numpy as np
import pytest

from mergeutil import BAD, C, D, T, assert_merge_is, cases, expected_merge, host_from_blocks
from pebble_amd import _native as N
from pebble_amd.merge import host_struct, merge_host
from scanutil import result_kvs

CASES = cases()


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_merge_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.MergeRunsC, N.MergeOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp and n == 11
    assert L.pbl_abi_version() == 9
    # the other lists are what they were
    assert L.pbl_scan_struct_layout(None, 0) == 15 and L.pbl_seek_struct_layout(None, 0) == 12


def test_workspace_bytes():
    L = N.lib()
    for nb in (0, 1, 1024, 1 << 20):
        prev = 0
        for nkv in (0, 1, 255, 256, 257, 1 << 20, 1 << 32):
            w = int(L.pbl_merge_workspace_bytes(4, nb, nkv))
            assert w % 16 == 0 and w >= prev and w >= 16 * nkv, (nb, nkv, w)
            assert w == int(L.pbl_merge_workspace_bytes(16, nb, nkv))  # nothing scales with the runs
            prev = w


class _Args:
    """A syntactically valid argument set over host memory posing as device
    memory: every call below must return before it touches any of it."""

    def __init__(self, n_runs=2):
        self.arr = np.zeros(64, np.uint64)
        p = self.arr.ctypes.data
        self.runs = (N.DecodeOutC * 16)()
        for d in self.runs:
            for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
                      "blk_key_base", "blk_val_base", "blk_status"):
                setattr(d, f, p)
        self.rs = N.MergeRunsC(ctypes.cast(self.runs, ctypes.POINTER(N.DecodeOutC)), n_runs, 4, D, 0, 100)
        o = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
                  "blk_key_base", "blk_val_base", "blk_status", "totals"):
            setattr(o, f, p)
        o.kv_cap = o.key_cap = o.val_cap = 8
        self.out = N.MergeOutC(o, p, p)
        self.ws_bytes = int(N.lib().pbl_merge_workspace_bytes(n_runs, 4, 100))
        self.ws = np.zeros(self.ws_bytes + 16, np.uint8)
        self.ws_ptr = (self.ws.ctypes.data + 15) // 16 * 16

    def batch(self, ws="own", ws_bytes=None, flags=0, rs="own", out="own"):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_merge_batch(ctypes.byref(self.rs) if rs == "own" else None,
                                       ctypes.byref(self.out) if out == "own" else None,
                                       ctypes.c_void_p(ptr) if ptr else None,
                                       self.ws_bytes if ws_bytes is None else ws_bytes, flags, None)

    def size(self, ws="own", ws_bytes=None, rs="own", out="own"):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_merge_size(ctypes.byref(self.rs) if rs == "own" else None,
                                      ctypes.byref(self.out) if out == "own" else None,
                                      ctypes.c_void_p(ptr) if ptr else None,
                                      self.ws_bytes if ws_bytes is None else ws_bytes, None)

    def host(self):
        return N.lib().pbl_merge_batch_host(ctypes.byref(self.rs), ctypes.byref(self.out))


def test_invalid_arguments_return_before_any_device_call():
    I = N.PBL_INVALID_ARG

    def bad(mut, calls=("batch", "size"), **kw):
        for call in calls:
            a = _Args()
            mut(a)
            assert getattr(a, call)(**kw) == I, (call, kw)

    both = ("batch", "size", "host")
    bad(lambda a: None, rs=None)
    bad(lambda a: None, out=None)
    bad(lambda a: setattr(a.rs, "runs", None), both)
    bad(lambda a: setattr(a.rs, "n_runs", 0), both)
    bad(lambda a: setattr(a.rs, "n_runs", 17), both)
    bad(lambda a: setattr(a.rs, "comparer", C + 1), both)
    for f in ("trailer", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base", "blk_val_base",
              "blk_status"):
        bad(lambda a, f=f: setattr(a.runs[1], f, None), both)  # a needed array of the last run
        bad(lambda a, f=f: setattr(a.runs[0], f, None), both)
    for f in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_status", "totals"):
        bad(lambda a, f=f: setattr(a.out.result, f, None), both)
    for f in ("trailer", "key_off", "val_off", "key_bytes", "val_bytes"):  # needed once anything can be written
        bad(lambda a, f=f: setattr(a.out.result, f, None), ("batch", "host"))
    # only one of the tiering arrays, in a run or in the result
    bad(lambda a: setattr(a.runs[1], "tiering_span_id", a.arr.ctypes.data), both)
    bad(lambda a: setattr(a.runs[0], "tiering_attr", a.arr.ctypes.data), both)
    bad(lambda a: setattr(a.out.result, "tiering_span_id", a.arr.ctypes.data), ("batch", "host"))
    bad(lambda a: setattr(a.out.result, "tiering_attr", a.arr.ctypes.data), ("batch", "host"))
    # the workspace: NULL, misaligned, one byte short
    bad(lambda a: None, ws=None)
    a = _Args()
    assert a.batch(ws=a.ws_ptr + 8) == I and a.size(ws=a.ws_ptr + 8) == I
    assert a.batch(ws_bytes=a.ws_bytes - 1) == I and a.size(ws_bytes=a.ws_bytes - 1) == I
    assert a.batch(flags=2) == I and a.batch(flags=N.PBL_MERGE_SIZED | 4) == I
    # a run past n_runs is not looked at
    a = _Args(n_runs=16)
    a.rs.n_runs = 3
    a.runs[3].trailer = None
    assert a.host() == N.PBL_OK  # (four empty blocks per run)
    assert not a.arr.any() and not a.ws.any()


@pytest.mark.parametrize("name,comparer,runs", CASES, ids=[c[0] for c in CASES])
def test_host_merge_equals_sorted(name, comparer, runs):
    hosts = [host_from_blocks(r) for r in runs]
    res = merge_host(hosts, comparer=comparer)
    assert_merge_is(res, hosts, comparer, name)
    # a merge result can be merged again: alone it comes back as it is
    again = merge_host([res[0]], comparer=comparer)
    for q in range(len(runs[0])):
        assert result_kvs(again[0], q) == result_kvs(res[0], q), (name, q)
    assert again[0]["blk_status"].tolist() == res[0]["blk_status"].tolist()


def test_case_list_covers_what_it_names():
    by = {c[0]: c for c in CASES}
    lens = {len(b) for name, _, runs in CASES if name.startswith("lengths") for r in runs for b in r}
    assert lens == {0, 1, 63, 64, 65, 255, 256, 257}
    assert [len(c[2]) for c in CASES[:4]] == [1, 2, 3, 16]
    kv = [x for r in by["key and value lengths"][2] for b in r for x in b]
    assert {len(k) for k, _, _ in kv} == {0, 1, 15, 16, 17, 200}
    assert {len(v) for _, _, v in kv} == {0, 1, 15, 16, 17, 511, 512, 513, 5000}


def test_ties_go_in_run_order():
    _, comparer, runs = next(c for c in CASES if c[0] == "equal internal keys")
    r, src_run, src_kv = merge_host([host_from_blocks(x) for x in runs], comparer=comparer)
    vals = [v for _, _, v, _ in result_kvs(r, 0)]
    assert vals[:3] == [b"run0 a9", b"run1 a9", b"run2 a9"]
    assert vals[3:9] == [b"run0 b5 first", b"run0 b5 second", b"run1 b5 first", b"run1 b5 second", b"run2 b5 first",
                         b"run2 b5 second"]
    assert src_run.tolist() == [0, 1, 2, 0, 0, 1, 1, 2, 2, 0, 1, 2] and src_kv.tolist() == [0, 0, 0, 1, 2, 1, 2, 1, 2, 3, 3, 3]


def test_comparers_decide_the_order():
    _, _, runs = next(c for c in CASES if c[0] == "testkeys suffixes")
    r = merge_host([host_from_blocks(x) for x in runs], comparer=T)[0]
    assert [(k, t >> 8) for k, t, _, _ in result_kvs(r, 0)] == [
        (b"a", 4), (b"a", 3), (b"a@10", 8), (b"a@10", 7), (b"a@7", 2), (b"a@5", 7), (b"a@5_synthetic", 7), (b"a@5", 6),
        (b"b", 9), (b"b@2", 1), (b"b@2", 1)]
    _, _, runs = next(c for c in CASES if c[0] == "crdb equal versions")
    r = merge_host([host_from_blocks(x) for x in runs], comparer=C)[0]
    assert [v for _, _, v, _ in result_kvs(r, 0)] == [
        b"r0 bare", b"r1 7,1", b"r0 7", b"r1 5,0", b"r0 5", b"r1 5,0,syn", b"r2 5,0,syn", b"r2 5", b"r0 k2",
        b"r2 k2 tie"]


def test_an_unsorted_block_is_reported_and_its_neighbours_are_merged():
    _, comparer, runs = next(c for c in CASES if c[0] == "unsorted block")
    hosts = [host_from_blocks(x) for x in runs]
    r = merge_host(hosts, comparer=comparer)[0]
    assert r["blk_status"].tolist() == [0, N.PBL_INVALID_ARG, 0] and r["status_mask"] == 1 << N.PBL_INVALID_ARG
    assert np.diff(r["blk_kv_base"]).tolist() == [40, 0, 44] and r["n_bad_blocks"] == 1
    _, comparer, runs = next(c for c in CASES if c[0] == "unsorted trailers")
    r = merge_host([host_from_blocks(x) for x in runs], comparer=comparer)[0]
    assert r["blk_status"].tolist() == [N.PBL_INVALID_ARG] and r["n_kv"] == 0


def test_a_bad_block_gives_its_status_to_the_result_block():
    _, comparer, runs = next(c for c in CASES if c[0] == "bad block")
    hosts = [host_from_blocks(x) for x in runs]
    r = merge_host(hosts, comparer=comparer)[0]
    assert r["blk_status"].tolist() == [0, BAD, 0] and r["status_mask"] == 1 << BAD and r["n_bad_blocks"] == 1
    assert np.diff(r["blk_kv_base"]).tolist() == [30, 0, 36]
    # the first non-OK status in run order
    hosts[2]["blk_status"][1] = N.PBL_CORRUPT_BOUNDS
    hosts[0]["blk_status"][2] = N.PBL_UNSUPPORTED
    r = merge_host(hosts, comparer=comparer)[0]
    assert r["blk_status"].tolist() == [0, BAD, N.PBL_UNSUPPORTED]
    assert expected_merge(hosts, comparer)[2][0] == N.PBL_UNSUPPORTED


def test_overflow_writes_sizes_and_nothing_else():
    _, comparer, runs = next(c for c in CASES if c[0] == "lengths K=3")
    hosts = [host_from_blocks(x) for x in runs]
    full = merge_host(hosts, comparer=comparer)[0]
    caps = (full["n_kv"], full["key_bytes_total"], full["val_bytes_total"])
    nb = len(runs[0])
    keep = []
    arr = (N.DecodeOutC * 3)(*[host_struct(h, keep) for h in hosts])
    rs = N.MergeRunsC(ctypes.cast(arr, ctypes.POINTER(N.DecodeOutC)), 3, nb, comparer, 0, 0)
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        a = {"trailer": np.full(caps[0], 0xAA, np.uint64), "kv_flags": np.full(caps[0], 0xAA, np.uint8),
             "key_off": np.full(caps[0] + nb, 0xAA, np.uint32), "val_off": np.full(caps[0] + nb, 0xAA, np.uint32),
             "key_bytes": np.full(caps[1], 0xAA, np.uint8), "val_bytes": np.full(caps[2], 0xAA, np.uint8)}
        fill = {k: v.copy() for k, v in a.items()}
        b = {k: np.zeros(nb + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base")}
        st = np.full(nb, 99, np.uint32)
        tot = N.TotalsC()
        o = N.DecodeOutC()
        for k, v in {**a, **b}.items():
            setattr(o, k, v.ctypes.data)
        o.blk_status = st.ctypes.data
        o.totals = ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap
        sr, sk = np.full(caps[0], 0xAA, np.uint8), np.full(caps[0], 0xAA, np.uint64)
        mo = N.MergeOutC(o, sr.ctypes.data, sk.ctypes.data)
        assert N.lib().pbl_merge_batch_host(ctypes.byref(rs), ctypes.byref(mo)) == N.PBL_OK
        assert tot.status_mask == 1 << N.PBL_OVERFLOW and (tot.n_kv, tot.key_bytes, tot.val_bytes) == caps, short
        for k in b:
            assert b[k].tolist() == full[k].tolist(), (short, k)
        assert st.tolist() == [0] * nb
        for k in a:
            assert (a[k] == fill[k]).all(), (short, k)
        assert (sr == 0xAA).all() and (sk == 0xAA).all()
