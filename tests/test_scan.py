"""Batched bounded scans without a GPU: the ABI additions
(pbl_scan_struct_layout, the workspace size, every invalid-argument return, all
before any device call) and pbl_scan_batch_host -- the same bounds_one the
device kernel instantiates, then a plain gather -- against a walk of the
one-key host iterator (scanutil.expected_scan) over the oracle's decoded
arrays: both modes, HideObsoletePoints on and off, the three comparers."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer
from pebble_amd.scan import pack_bounds, scan_host
from scanutil import assert_same, assert_scan_is, expected_scan, result_kvs
from seekutil import Seq, block_of, keyfn, sorted_keys, trailer_index


def decoded(blocks, flags=0):
    off, lens, pos = [], [], 0
    for b in blocks:
        off.append(pos)
        lens.append(len(b))
        pos += (len(b) + 15) // 16 * 16
    buf = np.zeros(pos + 16, np.uint8)
    for o, b in zip(off, blocks):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return oracle.rowblk_decode_batch(buf, np.array(off, np.uint64), np.array(lens, np.uint32), flags)


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_scan_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.ScanQueriesC, N.ScanOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp
    assert L.pbl_abi_version() == 9
    # the other two lists are what they were
    assert L.pbl_seek_struct_layout(None, 0) == 12
    assert L.pbl_struct_layout(None, 0) == L.pbl_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 0)


def test_workspace_bytes():
    L = N.lib()
    for nb in (0, 1, 1024, 1 << 20):
        prev = 0
        for nkv in (0, 1, 255, 256, 257, 1 << 20, 1 << 32):
            w = int(L.pbl_scan_workspace_bytes(7, nb, nkv))
            assert w % 16 == 0 and w >= prev and w >= int(L.pbl_seek_workspace_bytes(nb)), (nb, nkv, w)
            # 28 B per 256 KVs: no per-KV state
            assert w - int(L.pbl_scan_workspace_bytes(7, nb, 0)) <= 28 * (nkv // 256 + 1) + 64
            prev = w
    # per query a fixed number of bytes, whatever the ranges hold
    a, b = (int(L.pbl_scan_workspace_bytes(n, 16, 4096)) for n in (1000, 2000))
    assert 0 < b - a <= 1000 * 128


class _Args:
    """A syntactically valid argument set over host memory posing as device
    memory: every call below must return before it touches any of it."""

    def __init__(self):
        self.arr = np.zeros(64, np.uint64)
        p = self.arr.ctypes.data
        self.d = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
                  "blk_key_base", "blk_val_base", "blk_status"):
            setattr(self.d, f, p)
        self.q = N.ScanQueriesC(p, p, p, p, p, p, 4, N.PBL_CMP_DEFAULT, 0, 0)
        o = N.DecodeOutC()
        for f in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
                  "blk_key_base", "blk_val_base", "blk_status", "totals"):
            setattr(o, f, p)
        o.kv_cap = o.key_cap = o.val_cap = 8
        self.out = N.ScanOutC(o, p, p)
        self.ws_bytes = int(N.lib().pbl_scan_workspace_bytes(4, 4, 100))
        self.ws = np.zeros(self.ws_bytes + 16, np.uint8)
        self.ws_ptr = (self.ws.ctypes.data + 15) // 16 * 16

    def batch(self, ws="own", ws_bytes=None, flags=0):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_scan_batch(ctypes.byref(self.d), 4, 100, ctypes.byref(self.q), ctypes.byref(self.out),
                                      ctypes.c_void_p(ptr) if ptr else None,
                                      self.ws_bytes if ws_bytes is None else ws_bytes, flags, None)

    def size(self, ws_bytes=None):
        return N.lib().pbl_scan_size(ctypes.byref(self.d), 4, 100, ctypes.byref(self.q), ctypes.byref(self.out),
                                     ctypes.c_void_p(self.ws_ptr), self.ws_bytes if ws_bytes is None else ws_bytes,
                                     None)

    def prepare(self, comparer=0, hide=0, ws="own", ws_bytes=None):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_scan_prepare(ctypes.byref(self.d), 4, 100, comparer, hide,
                                        ctypes.c_void_p(ptr) if ptr else None,
                                        self.ws_bytes if ws_bytes is None else ws_bytes, None)


def test_invalid_arguments_return_before_any_device_call():
    L = N.lib()
    I = N.PBL_INVALID_ARG

    def bad(mut, call="batch", **kw):
        a = _Args()
        mut(a)
        assert getattr(a, call)(**kw) == I, (call, kw)

    bad(lambda a: setattr(a.q, "comparer", 3))
    bad(lambda a: setattr(a.q, "lower_off", None))
    bad(lambda a: setattr(a.q, "upper_off", None))
    bad(lambda a: setattr(a.q, "upper_bytes", None))
    bad(lambda a: setattr(a.d, "blk_status", None))
    bad(lambda a: setattr(a.d, "val_off", None))
    bad(lambda a: setattr(a.d, "trailer", None))
    bad(lambda a: setattr(a.d, "tiering_attr", a.arr.ctypes.data))   # one tiering array only
    bad(lambda a: (setattr(a.q, "hide_obsolete_points", 1), setattr(a.d, "kv_flags", None)))
    bad(lambda a: setattr(a.out.result, "blk_kv_base", None))
    bad(lambda a: setattr(a.out.result, "totals", None))
    bad(lambda a: setattr(a.out.result, "key_bytes", None))          # a capacity without its array
    bad(lambda a: None, ws=None)
    bad(lambda a: None, ws_bytes=_Args().ws_bytes - 1)
    bad(lambda a: None, flags=2)
    a = _Args()
    assert a.batch(ws=a.ws_ptr + 8) == I
    bad(lambda a: setattr(a.q, "comparer", 3), call="size")
    bad(lambda a: setattr(a.out.result, "blk_status", None), call="size")
    bad(lambda a: None, call="size", ws_bytes=_Args().ws_bytes - 1)
    bad(lambda a: None, call="prepare", comparer=3)
    bad(lambda a: None, call="prepare", ws=None)
    bad(lambda a: None, call="prepare", ws_bytes=int(L.pbl_scan_workspace_bytes(0, 4, 100)) - 1)
    bad(lambda a: setattr(a.d, "key_off", None), call="prepare")
    bad(lambda a: setattr(a.d, "kv_flags", None), call="prepare", hide=1)
    # the host entry point shares the checks
    a = _Args()
    a.q.comparer = 3
    assert L.pbl_scan_batch_host(ctypes.byref(a.d), 4, ctypes.byref(a.q), ctypes.byref(a.out)) == I
    a = _Args()
    a.d.val_bytes = None
    assert L.pbl_scan_batch_host(ctypes.byref(a.d), 4, ctypes.byref(a.q), ctypes.byref(a.out)) == I
    assert L.pbl_scan_batch_host(None, 4, ctypes.byref(a.q), ctypes.byref(a.out)) == I


def _ordered_batch(rng, comparer, n_blocks, seq):
    """Blocks whose user keys ascend over the whole batch (a table's data
    blocks), an empty block and a corrupt one in the middle."""
    kf = keyfn(rng, comparer, roaches=(b"k1", b"k2", b"k3", b"k4", b"k5"))
    keys = sorted_keys(comparer, [kf() for _ in range(40 * n_blocks)])
    cuts = sorted(rng.sample(range(1, len(keys)), n_blocks - 1))
    parts = [keys[a:b] for a, b in zip([0] + cuts, cuts + [len(keys)])]
    blocks = [block_of(rng, seq, p) for p in parts]
    blocks.insert(2, Writer(16).finish())       # decodes, holds nothing
    blocks.insert(4, b"\x00\x00\x00\x00")       # zero restarts: PBL_CORRUPT_NO_RESTARTS
    return blocks, keys, kf


def _bounds(rng, keys, kf, n):
    """Ranges between existing keys, absent keys, None and empty bounds; some inverted."""
    pool = keys + [kf() for _ in range(30)]
    lo = [rng.choice(pool + [None, b""]) for _ in range(n)]
    up = [rng.choice(pool + [None, None, b""]) for _ in range(n)]
    return lo, up


@pytest.mark.parametrize("comparer", [N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB])
def test_host_scan_matches_the_iterator_walk(comparer):
    rng = random.Random(comparer + 41)
    blocks, keys, kf = _ordered_batch(rng, comparer, 6, Seq())
    d = decoded(blocks)
    assert int(d["blk_status"][4]) != 0 and int(d["blk_status"][2]) == 0
    nb = len(blocks)
    tidx = trailer_index(d)
    lo, up = _bounds(rng, keys, kf, 120)
    lo += [None, keys[0], keys[-1], keys[5]]
    up += [None, keys[-1], None, keys[5]]
    for hide in (False, True):
        got = scan_host(d, lo, up, comparer=comparer, hide_obsolete_points=hide)
        assert_scan_is(got, expected_scan(d, lo, up, comparer, None, hide, tidx), comparer, (comparer, hide, "table"))
        blk = [rng.randrange(nb + 2) for _ in lo]  # past-the-end ids and the corrupt block too
        got = scan_host(d, lo, up, comparer=comparer, blocks=blk, hide_obsolete_points=hide)
        exp = expected_scan(d, lo, up, comparer, blk, hide, tidx)
        assert_scan_is(got, exp, comparer, (comparer, hide, "block"))
        st = got[0]["blk_status"]
        for i, b in enumerate(blk):
            if b >= nb:
                assert int(st[i]) == N.PBL_INVALID_ARG
            elif b == 4:
                assert int(st[i]) == int(d["blk_status"][4])
    # the whole table, unbounded: every KV of every PBL_OK block, across the corrupt one
    r, rng_, src = scan_host(d, [None], [None], comparer=comparer)
    assert src.tolist() == list(range(d["n_kv"])) and rng_.tolist() == [[0, d["n_kv"]]]


def test_host_scan_empty_inverted_and_no_upper():
    rng = random.Random(3)
    C = N.PBL_CMP_DEFAULT
    keys = [b"k%03d" % i for i in range(80)]
    seq = Seq()
    d = decoded([block_of(rng, seq, keys[:40], obsolete=0.0), block_of(rng, seq, keys[40:], obsolete=0.0)])
    n = d["n_kv"]
    k = keys[10]
    lo = [k, keys[50], b"", None, k, b"\xff\xff", k, None]
    up = [k, keys[20], b"", b"", None, None, b"", keys[0]]
    r, rg, src = got = scan_host(d, lo, up, comparer=C)
    sizes = np.diff(r["blk_kv_base"]).tolist()
    first_k = min(i for i in range(n) if _key(d, i) >= k)
    # [k, k), inverted, ["", ""), [First, ""), [k, +inf), past the end, [k, "") (an empty upper key is a
    # bound, not "none"), [First, first key)
    assert sizes == [0, 0, 0, 0, n - first_k, 0, 0, 0]
    assert (rg[:, 0] <= rg[:, 1]).all() and rg[4].tolist() == [first_k, n]
    assert r["status_mask"] == 0 and (r["blk_status"] == 0).all()
    assert_scan_is(got, expected_scan(d, lo, up, C), C)
    fl = pack_bounds(lo, up)[4]
    assert fl.tolist() == [0, 0, 0, 0, 1, 1, 0, 0]


def _key(d, i):
    b = int(np.searchsorted(d["blk_kv_base"], i, side="right")) - 1
    o = d["key_off"][i + b: i + b + 2].astype(np.int64) + int(d["blk_key_base"][b])
    return d["key_bytes"][o[0]:o[1]].tobytes()


def test_host_scan_duplicate_and_overlapping_queries():
    rng = random.Random(9)
    C = N.PBL_CMP_DEFAULT
    keys = [b"k%03d" % i for i in range(100)]
    seq = Seq()
    d = decoded([block_of(rng, seq, keys[i:i + 20]) for i in range(0, len(keys), 20)])
    lo = [keys[5], keys[5], keys[10], None, keys[30]]
    up = [keys[60], keys[60], keys[40], None, keys[31]]
    for hide in (False, True):
        got = scan_host(d, lo, up, comparer=C, hide_obsolete_points=hide)
        assert_scan_is(got, expected_scan(d, lo, up, C, None, hide), C, hide)
        r = got[0]
        assert result_kvs(r, 0) == result_kvs(r, 1) and len(result_kvs(r, 0)) > 0
        assert r["n_kv"] > (d["n_kv"] if not hide else 0)  # more out than in: each query has its own copy
    # one query twice the other way round: the same result in another order
    fwd = scan_host(d, lo, up, comparer=C)
    rev = scan_host(d, lo[::-1], up[::-1], comparer=C)
    assert [result_kvs(rev[0], 4 - q) for q in range(5)] == [result_kvs(fwd[0], q) for q in range(5)]
    assert_same(fwd, scan_host(d, lo, up, comparer=C))


def test_host_scan_hidden_runs_cross_blocks():
    """Block 0's last two KVs, all of block 1 and block 2's first KV obsolete."""
    seq = Seq()

    def blk(keys, obs):
        w = Writer(2)
        for k, o in zip(keys, obs):
            w.add_with_optional_value_prefix(k, seq.next(), o, b"v" + k, len(k), False, 0, False)
        return w.finish()

    b0, b1, b2 = [b"a1", b"a2", b"a3", b"a4"], [b"b1", b"b2", b"b3"], [b"c1", b"c2", b"c3"]
    d = decoded([blk(b0, [0, 0, 1, 1]), blk(b1, [1, 1, 1]), blk(b2, [1, 0, 0])])
    C = N.PBL_CMP_DEFAULT
    r, rg, src = scan_host(d, [b"a2", b"a3", None], [b"c3", b"c2", None], comparer=C, hide_obsolete_points=True)
    assert src.tolist() == [1, 8] + [] + [0, 1, 8, 9]  # [a2, c3) = a2 c2; [a3, c2): all hidden; everything
    assert rg.tolist() == [[1, 9], [2, 8], [0, 10]]
    assert np.diff(r["blk_kv_base"]).tolist() == [2, 0, 4]
    r, _, src = scan_host(d, [b"a1", b""], [None, None], comparer=C, blocks=[1, 2], hide_obsolete_points=True)
    assert src.tolist() == [8, 9] and np.diff(r["blk_kv_base"]).tolist() == [0, 2]
    pts = [None] + b0 + b1 + b2 + [b"d"]
    lo = [a for a in pts for _ in pts]
    up = [b for _ in pts for b in pts]
    for hide in (False, True):
        assert_scan_is(scan_host(d, lo, up, comparer=C, hide_obsolete_points=hide),
                       expected_scan(d, lo, up, C, None, hide), C, hide)
        for b in range(3):
            assert_scan_is(scan_host(d, lo, up, comparer=C, blocks=[b] * len(lo), hide_obsolete_points=hide),
                           expected_scan(d, lo, up, C, [b] * len(lo), hide), C, (b, hide))


def test_host_scan_overflow_writes_sizes_only():
    rng = random.Random(11)
    C = N.PBL_CMP_DEFAULT
    keys = [b"k%03d" % i for i in range(30)]
    d = decoded([block_of(rng, Seq(), keys, obsolete=0.0)])
    full, _, _ = scan_host(d, [None, keys[3]], [None, keys[9]], comparer=C)
    caps = (full["n_kv"], full["key_bytes_total"], full["val_bytes_total"])
    assert min(caps) > 0
    lb, lo, ub, uo, fl = pack_bounds([None, keys[3]], [None, keys[9]])
    keep = {k: np.ascontiguousarray(d[k]) for k in ("trailer", "kv_flags", "key_off", "val_off", "key_bytes",
                                                     "val_bytes", "blk_kv_base", "blk_key_base", "blk_val_base",
                                                     "blk_status")}
    src = N.DecodeOutC()
    for k, a in keep.items():
        setattr(src, k, a.ctypes.data)
    q = N.ScanQueriesC(lb.ctypes.data, lo.ctypes.data, ub.ctypes.data, uo.ctypes.data, fl.ctypes.data, None, 2, C, 0,
                       0)
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        arr = {"trailer": np.full(caps[0], 0xAA, np.uint64), "kv_flags": np.full(caps[0], 0xAA, np.uint8),
               "key_off": np.full(caps[0] + 2, 0xAA, np.uint32), "val_off": np.full(caps[0] + 2, 0xAA, np.uint32),
               "key_bytes": np.full(caps[1], 0xAA, np.uint8), "val_bytes": np.full(caps[2], 0xAA, np.uint8)}
        base = {k: np.zeros(3, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base")}
        st = np.zeros(2, np.uint32)
        tot = N.TotalsC()
        o = N.DecodeOutC()
        for k, a in {**arr, **base}.items():
            setattr(o, k, a.ctypes.data)
        o.blk_status, o.totals = st.ctypes.data, ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap
        so = N.ScanOutC(o, None, None)
        assert N.lib().pbl_scan_batch_host(ctypes.byref(src), 1, ctypes.byref(q), ctypes.byref(so)) == N.PBL_OK
        assert tot.status_mask == 1 << N.PBL_OVERFLOW and (tot.n_kv, tot.key_bytes, tot.val_bytes) == caps
        for k in base:
            assert base[k].tolist() == full[k].tolist(), (short, k)
        for k, a in arr.items():
            assert (a == 0xAA).all(), (short, k)  # the sentinel: nothing written
