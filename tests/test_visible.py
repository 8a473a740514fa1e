"""The snapshot-visible view without a GPU: the ABI additions
(pbl_visible_struct_layout, the workspace size, every invalid-argument return,
all before any device call) and pbl_visible_batch_host -- the sequential state
machine -- against the Python statement of the rules
(visibleutil.expected_visible) on the hand-built cases and against the
reference's own iterator test data (tests/golden/iterator_points.json)."""
import ctypes

import numpy as np
import pytest

from mergeutil import BAD, C
from pebble_amd import _native as N
from pebble_amd.merge import host_struct
from pebble_amd.visible import SEQNUM_MAX, visible_host
from scanutil import result_kvs
from visibleutil import (D, MAX, assert_visible_is, cases, expected_visible, fold, golden_block, host_from_blocks, load_golden,
                         one_key_block, replay)

CASES = cases()
KEEP = N.PBL_VISIBLE_KEEP_OPERANDS


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_visible_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.VisibleInC, N.VisibleOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp and n == 10
    assert L.pbl_abi_version() == 9 and SEQNUM_MAX == (1 << 56) - 1
    # the other lists are what they were
    assert L.pbl_merge_struct_layout(None, 0) == 11 and L.pbl_scan_struct_layout(None, 0) == 15


def test_workspace_bytes():
    L = N.lib()
    for nb in (0, 1, 1024, 1 << 20):
        prev = 0
        for nkv in (0, 1, 255, 256, 257, 1 << 20, 1 << 32):
            w = int(L.pbl_visible_workspace_bytes(nb, nkv))
            assert w % 16 == 0 and w >= prev and w >= 41 * nkv, (nb, nkv, w)
            prev = w


class _Args:
    """A syntactically valid argument set over host memory posing as device
    memory: every call below must return before it touches any of it."""

    def __init__(self):
        self.arr = np.zeros(64, np.uint64)
        p = self.arr.ctypes.data
        d = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base",
                  "blk_val_base", "blk_status"):
            setattr(d, f, p)
        self.vin = N.VisibleInC(d, 4, D, 100, MAX)
        o = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base",
                  "blk_val_base", "blk_status", "totals"):
            setattr(o, f, p)
        o.kv_cap = o.key_cap = o.val_cap = 8
        self.out = N.VisibleOutC(o, p, p)
        self.ws_bytes = int(N.lib().pbl_visible_workspace_bytes(4, 100))
        self.ws = np.zeros(self.ws_bytes + 16, np.uint8)
        self.ws_ptr = (self.ws.ctypes.data + 15) // 16 * 16

    def batch(self, ws="own", ws_bytes=None, flags=0, vin="own", out="own"):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_visible_batch(ctypes.byref(self.vin) if vin == "own" else None,
                                         ctypes.byref(self.out) if out == "own" else None,
                                         ctypes.c_void_p(ptr) if ptr else None,
                                         self.ws_bytes if ws_bytes is None else ws_bytes, flags, None)

    def size(self, ws="own", ws_bytes=None, flags=0, vin="own", out="own"):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_visible_size(ctypes.byref(self.vin) if vin == "own" else None,
                                        ctypes.byref(self.out) if out == "own" else None,
                                        ctypes.c_void_p(ptr) if ptr else None,
                                        self.ws_bytes if ws_bytes is None else ws_bytes, flags, None)

    def host(self, flags=0, vin="own", out="own"):
        return N.lib().pbl_visible_batch_host(ctypes.byref(self.vin) if vin == "own" else None,
                                              ctypes.byref(self.out) if out == "own" else None, flags)


def test_invalid_arguments_return_before_any_device_call():
    I = N.PBL_INVALID_ARG

    def bad(mut, calls=("batch", "size", "host"), **kw):
        for call in calls:
            a = _Args()
            mut(a)
            assert getattr(a, call)(**kw) == I, (call, kw)

    bad(lambda a: None, vin=None)
    bad(lambda a: None, out=None)
    bad(lambda a: setattr(a.vin, "comparer", C + 1))
    for f in ("trailer", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base", "blk_key_base", "blk_val_base",
              "blk_status"):
        bad(lambda a, f=f: setattr(a.vin.batch, f, None))
    for f in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_status", "totals"):
        bad(lambda a, f=f: setattr(a.out.result, f, None))
    for f in ("trailer", "key_off", "val_off", "key_bytes", "val_bytes"):  # needed once anything can be written
        bad(lambda a, f=f: setattr(a.out.result, f, None), ("batch", "host"))
    # only one of the tiering arrays, in the input or in the result
    bad(lambda a: setattr(a.vin.batch, "tiering_span_id", a.arr.ctypes.data))
    bad(lambda a: setattr(a.vin.batch, "tiering_attr", a.arr.ctypes.data))
    bad(lambda a: setattr(a.out.result, "tiering_span_id", a.arr.ctypes.data), ("batch", "host"))
    bad(lambda a: setattr(a.out.result, "tiering_attr", a.arr.ctypes.data), ("batch", "host"))
    # the workspace: NULL, misaligned, one byte short
    bad(lambda a: None, ("batch", "size"), ws=None)
    a = _Args()
    assert a.batch(ws=a.ws_ptr + 8) == I and a.size(ws=a.ws_ptr + 8) == I
    assert a.batch(ws_bytes=a.ws_bytes - 1) == I and a.size(ws_bytes=a.ws_bytes - 1) == I
    # unknown flags; SIZED belongs to pbl_visible_batch alone
    assert a.batch(flags=4) == I and a.batch(flags=N.PBL_VISIBLE_SIZED | 8) == I
    assert a.size(flags=N.PBL_VISIBLE_SIZED) == I and a.size(flags=4) == I
    assert a.host(flags=N.PBL_VISIBLE_SIZED) == I and a.host(flags=4) == I
    assert a.host(flags=KEEP) == N.PBL_OK  # (four empty blocks)
    assert not a.arr.any() and not a.ws.any()


PARAMS = [(name, comparer, blocks, s, keep) for name, comparer, blocks, snaps in CASES for s in snaps
          for keep in (False, True)]
IDS = ["%s-%s%s" % (p[0], "max" if p[3] == MAX else p[3], "-keep" if p[4] else "") for p in PARAMS]


@pytest.mark.parametrize("name,comparer,blocks,snapshot,keep", PARAMS, ids=IDS)
def test_host_equals_the_python_model(name, comparer, blocks, snapshot, keep):
    h = host_from_blocks(blocks)
    res = visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep)
    exp = assert_visible_is(res, h, comparer, snapshot, keep, name)
    if keep:  # folding the operands reproduces the default mode's results
        folded = expected_visible(h, comparer, snapshot, False)
        for (st, e), (st2, f) in zip(exp, folded):
            if st == 0 and st2 == 0:
                assert fold(e) == f, name
    # a result is sorted with one visible version per key: it comes back as it is
    again = visible_host(res[0], comparer=comparer)
    for q in range(len(blocks)):
        if not keep:
            assert result_kvs(again[0], q) == result_kvs(res[0], q), (name, q)


def test_one_key_with_70000_versions():
    h = host_from_blocks([one_key_block()])
    for snapshot, n in ((MAX, 70000), (35001, 35000)):
        r, src_kv, n_src = visible_host(h, comparer=D, snapshot=snapshot)
        (k, t, v, f), = result_kvs(r, 0)
        assert (k, t >> 8, t & 0xff) == (b"the key", n, 2) and n_src.tolist() == [n] and src_kv.tolist() == [70000 - n]
        assert v == bytes(s % 251 for s in range(1, n + 1))
        assert_visible_is((r, src_kv, n_src), h, D, snapshot, False)


def test_case_list_covers_what_it_names():
    by = {c[0]: c for c in CASES}
    blk = by["wave and tile edges"][2][0]
    starts = [j for j in range(len(blk)) if j == 0 or blk[j][0] != blk[j - 1][0]]
    assert {63, 64, 65, 255, 256, 257} <= set(starts)
    exp = expected_visible(host_from_blocks(by["long invisible prefix"][2]), D, 1000)[0][1]
    assert [x[2] for x in exp] == [b"v4,", b"seen", b"v6,v7,v8,"] and exp[1][4] == 602
    exp = expected_visible(host_from_blocks(by["long chains"][2]), D)[0][1]
    assert [(x[0], x[5], len(x[2])) for x in exp] == [(b"a", 700, 700), (b"b", 700, 700), (b"c", 700, 700)]
    vals = [x for b in by["value lengths"][2] for x in b]
    for kind in (1, 2):
        assert {len(v) for _, t, v in vals if t & 0xff == kind} >= {0, 1, 15, 16, 17, 511, 512, 513, 5000}
    sts = [st for st, _ in expected_visible(host_from_blocks(by["statuses"][2]), D)]
    U, A = N.PBL_UNSUPPORTED, N.PBL_INVALID_ARG
    assert sts == [0, BAD, 0, A, 0, A, 0, U, 0, U, 0, U, 0, U, 0]
    assert [st for st, _ in expected_visible(host_from_blocks(by["statuses"][2]), D, MAX, True)][-2:] == [0, 0]
    # one group under the comparer, several under bytes; the head's bytes come out
    tk = by["testkeys equal suffixes"]
    e = expected_visible(host_from_blocks(tk[2]), tk[1])[0][1]
    assert [(x[0], x[2]) for x in e] == [(b"a@5", b"oldestmiddlenewest")]
    e = expected_visible(host_from_blocks(tk[2]), D)[0][1]
    assert [(x[0], x[2]) for x in e] == [(b"a@5", b"newest"), (b"a@5_synthetic", b"oldestmiddle"),
                                         (b"b@2_synthetic", b"shadowed under testkeys")]
    ck = by["crdb equal versions"]
    e = expected_visible(host_from_blocks(ck[2]), ck[1])[0][1]
    assert [x[2] for x in e] == [b"wall onlyzero logicalsyn", b"k2"] and e[0][0] == ck[2][0][0][0]
    assert len(expected_visible(host_from_blocks(ck[2]), D)[0][1]) == 4


def test_snapshot_zero_sees_nothing():
    _, comparer, blocks, snaps = next(c for c in CASES if c[0] == "snapshot sweep")
    assert snaps[:2] == [0, 1] and snaps[-1] == MAX
    r = visible_host(host_from_blocks(blocks), comparer=comparer, snapshot=0)[0]
    assert r["n_kv"] == 0 and r["status_mask"] == 0 and r["blk_status"].tolist() == [0, 0, 0]
    # the batch bit is not interpreted: such a sequence number is merely large
    h = host_from_blocks([[(b"a", ((1 << 55) | 3) << 8 | 1, b"batch"), (b"a", 2 << 8 | 1, b"committed")]])
    assert [x[2] for x in result_kvs(visible_host(h, comparer=D, snapshot=10)[0], 0)] == [b"committed"]
    assert [x[2] for x in result_kvs(visible_host(h, comparer=D)[0], 0)] == [b"batch"]


def test_golden_iterator_cases():
    g = load_golden()
    assert len(g["cases"]) >= 45 and sum(len(c["expected"]) for c in g["cases"]) >= 102
    assert sum(1 for c in g["cases"] if any(kv[2] == "MERGE" for kv in c["define"])) >= 15
    for i, c in enumerate(g["cases"]):
        h = host_from_blocks([golden_block(c, g["kinds"])])
        r = visible_host(h, comparer=D, snapshot=c["seq"])[0]
        assert r["status_mask"] == 0, i
        kvs = [(k, v) for k, _, v, _ in result_kvs(r, 0)]
        assert replay(kvs, c["commands"]) == c["expected"], (i, c)


def test_overflow_writes_sizes_and_nothing_else():
    _, comparer, blocks, _ = next(c for c in CASES if c[0] == "wave and tile edges")
    h = host_from_blocks(blocks)
    full = visible_host(h, comparer=comparer)[0]
    caps = (full["n_kv"], full["key_bytes_total"], full["val_bytes_total"])
    nb = len(blocks)
    keep = []
    vin = N.VisibleInC(host_struct(h, keep), nb, comparer, 0, MAX)
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
        sk, ns = np.full(caps[0], 0xAA, np.uint64), np.full(caps[0], 0xAA, np.uint32)
        vo = N.VisibleOutC(o, sk.ctypes.data, ns.ctypes.data)
        assert N.lib().pbl_visible_batch_host(ctypes.byref(vin), ctypes.byref(vo), 0) == N.PBL_OK
        assert tot.status_mask == 1 << N.PBL_OVERFLOW and (tot.n_kv, tot.key_bytes, tot.val_bytes) == caps, short
        for k in b:
            assert b[k].tolist() == full[k].tolist(), (short, k)
        assert st.tolist() == [0] * nb
        for k in a:
            assert (a[k] == fill[k]).all(), (short, k)
        assert (sk == 0xAA).all() and (ns == 0xAA).all()


def test_meta_and_entry_offsets_travel_with_the_head():
    _, comparer, blocks, _ = next(c for c in CASES if c[0] == "wave and tile edges")
    h = host_from_blocks(blocks)
    n = h["n_kv"]
    h["entry_off"] = np.arange(n, dtype=np.uint32) * 7
    h["tiering_span_id"] = np.arange(n, dtype=np.uint64) + 1000
    h["tiering_attr"] = np.arange(n, dtype=np.uint64) * 3
    for keep in (False, True):
        r, src_kv, _ = visible_host(h, comparer=comparer, snapshot=2500, keep_operands=keep)
        at = src_kv.astype(np.int64)
        assert r["n_kv"] > 0
        for k in ("entry_off", "tiering_span_id", "tiering_attr", "trailer"):
            assert (r[k] == h[k][at]).all(), (k, keep)
