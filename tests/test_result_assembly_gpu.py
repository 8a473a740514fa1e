"""The code that the batched scan, merge and visible view share to assemble a
result (pebble_amd/csrc/result_core.hip.h), driven through all three operators
at the sizes where it takes another path: more than one chunk of 256 result
blocks, more than 256 tiles, value lengths around both copy forms in one wave,
sources without the optional per-KV arrays, and a capacity overflow found by
the last of three chunks.  The inputs are laid out as host arrays and uploaded,
so that statuses, flags and missing arrays are exactly what a case says.  Every
case compares every array of the device result with the operator's
*_batch_host result (a different algorithm) on the same input."""
import ctypes
import functools

import numpy as np
import pytest

import mergeutil
import scanutil
import visibleutil
from mergeutil import BAD, host_from_blocks
from pebble_amd import _native as N
from pebble_amd.merge import merge, merge_host
from pebble_amd.scan import pack_bounds, prepare, scan, scan_host
from pebble_amd.visible import visible, visible_host
from scanutil import ARRAYS, TOTALS, result_kvs

pytestmark = pytest.mark.gpu

D = N.PBL_CMP_DEFAULT
MAX = N.PBL_SEQNUM_MAX
SET, MERGE = 1, 2
EDGES = (255, 256, 257, 511, 512, 600)  # the bases looked at one by one: around both chunk edges, and the end
VALUE_LENGTHS = [0, 1, 15, 16, 17, 127, 128, 129, 512, 513, 1025]
HANDLE_BITS = N.PBL_KV_VALBLK_HANDLE | N.PBL_KV_BLOB_HANDLE


def T(seq, kind=SET):
    return seq << 8 | kind


def value(i, n):
    return bytes((7 * i + t) & 0xff for t in range(n))


def upload(h):
    """A host batch (to_host()'s layout) as a DecodedBatch on the device."""
    import torch
    from pebble_amd.batch import Capacity, DecodedBatch
    nb = len(h["blk_status"])
    d = DecodedBatch.allocate(nb, Capacity(h["n_kv"], h["key_bytes_total"], h["val_bytes_total"], 0), "cuda",
                              entry_off=h.get("entry_off") is not None, restarts=False,
                              meta=h.get("tiering_span_id") is not None)
    tot = N.TotalsC(h["n_kv"], h["key_bytes_total"], h["val_bytes_total"], 0, h["status_mask"], h["n_bad_blocks"], 0, 0)
    arrays = dict(h, totals=np.frombuffer(bytes(tot), np.uint8))
    for k in ("trailer", "kv_flags", "entry_off", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
              "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status", "totals", "tiering_span_id", "tiering_attr"):
        a = arrays.get(k)
        if a is not None and a.size:
            a = np.ascontiguousarray(a).view(np.uint8)
            getattr(d, k).view(torch.uint8)[: a.size].copy_(torch.from_numpy(a.copy()))
    torch.cuda.synchronize()
    d.read_totals()
    return d


def same_arrays(got, exp, ctx):
    for k in ARRAYS:
        x, y = np.asarray(got[k]), np.asarray(exp[k])
        assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k)
    for k in TOTALS:
        assert int(got[k]) == int(exp[k]), (ctx, k, got[k], exp[k])


def check_bases(r, counts, ctx):
    """The result's KV bases against the per-block counts the case was built
    with (independent of both implementations), index by index at EDGES."""
    base = np.concatenate(([0], np.cumsum(np.asarray(counts, np.uint64)))).astype(np.uint64)
    for i in EDGES:
        assert int(r["blk_kv_base"][i]) == int(base[i]), (ctx, "blk_kv_base", i)
        for k in ("blk_key_base", "blk_val_base"):
            assert int(r[k][i]) >= int(r[k][i - 1]), (ctx, k, i)
    assert r["blk_kv_base"].tolist() == base.tolist(), ctx
    assert r["n_kv"] == int(base[-1]) and int(r["blk_key_base"][600]) == r["key_bytes_total"] == len(r["key_bytes"]), ctx
    assert int(r["blk_val_base"][600]) == r["val_bytes_total"] == len(r["val_bytes"]), ctx


# ---- the 600-block inputs: three chunks, one block that is not PBL_OK in each ----------------------
NB = 600
BAD_AT = (100, 300, 580)


def _block(q, n, r=0):
    return [(b"q%03d-%d" % (q, 2 * j + r), T(1000 + q), value(q + j, (q + 3 * j + r) % 5)) for j in range(n)]


@functools.lru_cache(maxsize=None)
def merge_inputs():
    """Two runs whose result blocks hold 0 to 3 KVs; block 100 is corrupt in run
    1, block 300 unsorted in run 0, block 580 corrupt in run 0."""
    runs = [[_block(q, q % 3, 0) for q in range(NB)], [_block(q, (q // 3) % 2, 1) for q in range(NB)]]
    runs[1][100] = None
    runs[0][300] = _block(300, 2, 0)[::-1]
    runs[0][580] = None
    hosts = [host_from_blocks(b) for b in runs]
    counts = [0 if q in BAD_AT else q % 3 + (q // 3) % 2 for q in range(NB)]
    return hosts, merge_host(hosts, comparer=D), counts


@functools.lru_cache(maxsize=None)
def single_input():
    """One batch whose blocks hold 0 to 3 KVs, all of distinct user keys; block
    100 is corrupt, block 300 unsorted, block 580 holds a kind the view does
    not take (the scan copies the last two as they are)."""
    blocks = [_block(q, (7 * q + 3) % 4) for q in range(NB)]
    blocks[100] = None
    blocks[300] = _block(300, 3)[::-1]
    blocks[580] = [(b"q580", T(5, 21), b"x")]
    h = host_from_blocks(blocks)
    return h, blocks


@functools.lru_cache(maxsize=None)
def visible_inputs():
    h, blocks = single_input()
    counts = [0 if q in BAD_AT else len(blocks[q]) for q in range(NB)]
    return h, visible_host(h, comparer=D), counts


@functools.lru_cache(maxsize=None)
def scan_inputs():
    """600 per-block queries, query i over block i; query 300 names a block past the end."""
    h, blocks = single_input()
    ids = [9999 if q == 300 else q for q in range(NB)]
    lo, up = [None] * NB, [None] * NB
    counts = [0 if q in (100, 300) else len(blocks[q]) for q in range(NB)]
    return h, (lo, up, ids), scan_host(h, lo, up, comparer=D, blocks=ids), counts


def test_three_chunks_merge():
    hosts, exp, counts = merge_inputs()
    assert exp[0]["n_kv"] == sum(counts) and 0 in counts and 3 in counts
    r = mergeutil.device_result(merge([upload(h) for h in hosts], comparer=D))
    mergeutil.assert_same(r, exp, "merge, three chunks")
    check_bases(r[0], counts, "merge")
    assert r[0]["n_bad_blocks"] == 3 and r[0]["status_mask"] == 1 << BAD | 1 << N.PBL_INVALID_ARG
    assert [int(r[0]["blk_status"][q]) for q in BAD_AT] == [BAD, N.PBL_INVALID_ARG, BAD]


def test_three_chunks_visible():
    h, exp, counts = visible_inputs()
    assert exp[0]["n_kv"] == sum(counts) and 0 in counts and 3 in counts
    r = visibleutil.device_result(visible(upload(h), comparer=D))
    visibleutil.assert_same(r, exp, "visible, three chunks")
    check_bases(r[0], counts, "visible")
    assert r[0]["n_bad_blocks"] == 3
    assert r[0]["status_mask"] == 1 << BAD | 1 << N.PBL_INVALID_ARG | 1 << N.PBL_UNSUPPORTED
    assert [int(r[0]["blk_status"][q]) for q in BAD_AT] == [BAD, N.PBL_INVALID_ARG, N.PBL_UNSUPPORTED]


def test_three_chunks_scan():
    h, (lo, up, ids), exp, counts = scan_inputs()
    assert exp[0]["n_kv"] == sum(counts)
    r = scanutil.device_result(scan(upload(h), lo, up, comparer=D, blocks=ids))
    scanutil.assert_same(r, exp, "scan, three chunks")
    check_bases(r[0], counts, "scan")
    assert r[0]["n_bad_blocks"] == 2 and r[0]["status_mask"] == 1 << BAD | 1 << N.PBL_INVALID_ARG
    assert [int(r[0]["blk_status"][q]) for q in BAD_AT] == [BAD, N.PBL_INVALID_ARG, 0]


# ---- value lengths around both copy forms, short and long ones in one wave --------------------------
def test_value_copy_edges_merge():
    """44 result KVs, so one wave holds them all: values of at most 512 B and
    longer ones side by side, from both runs."""
    n = 2 * len(VALUE_LENGTHS)
    runs = [[[(b"v%03d" % (2 * i + r), T(50 + i), value(i + 100 * r, VALUE_LENGTHS[(i + 5 * r) % len(VALUE_LENGTHS)]))
              for i in range(n)]] for r in (0, 1)]
    hosts = [host_from_blocks(b) for b in runs]
    r = mergeutil.device_result(merge([upload(h) for h in hosts], comparer=D))
    mergeutil.assert_same(r, merge_host(hosts, comparer=D), "merge, value lengths")
    assert r[0]["n_kv"] == 2 * n <= 64
    exp = sorted(kv for run in runs for kv in run[0])
    assert [(k, t, v) for k, t, v, _ in result_kvs(r[0], 0)] == exp
    lens = {len(kv[2]) for kv in exp}
    assert lens == set(VALUE_LENGTHS)


@pytest.mark.parametrize("keep", [False, True], ids=["folded", "keep_operands"])
def test_value_copy_edges_visible(keep):
    """One block under 64 KVs: a SET of every length, and a MERGE chain with a
    513-B operand over a 1025-B SET."""
    kvs = [(b"a%03d" % i, T(50 + i), value(i, n)) for i, n in enumerate(VALUE_LENGTHS)]
    chain = [(b"m", T(9, MERGE), value(9, 513)), (b"m", T(8, MERGE), value(8, 17)), (b"m", T(7, SET), value(7, 1025)),
             (b"m", T(6, SET), b"shadowed")]
    tail = [(b"z%03d" % i, T(50 + i), value(i + 40, n)) for i, n in enumerate(reversed(VALUE_LENGTHS))]
    block = kvs + chain + tail
    assert len(block) < 64
    h = host_from_blocks([block])
    r = visibleutil.device_result(visible(upload(h), comparer=D, keep_operands=keep))
    visibleutil.assert_same(r, visible_host(h, comparer=D, keep_operands=keep), ("visible, value lengths", keep))
    got = [(k, t, v) for k, t, v, _ in result_kvs(r[0], 0)]
    folded = (b"m", T(9, MERGE), chain[2][2] + chain[1][2] + chain[0][2])  # oldest first
    assert got == kvs + (chain[:3] if keep else [folded]) + tail
    assert r[2].tolist() == [1] * len(kvs) + ([3, 0, 0] if keep else [3]) + [1] * len(tail)


# ---- more than 256 tiles ---------------------------------------------------------------------------
N_RUN = 33100


def test_more_than_256_tiles_merge():
    """66 200 result KVs are 259 tiles: the one-workgroup tile scan takes two steps."""
    runs = [[[(b"%06d" % (2 * i + r), T(7), bytes([(i + r) & 0xff])) for i in range(N_RUN)]] for r in (0, 1)]
    hosts = [host_from_blocks(b) for b in runs]
    r = mergeutil.device_result(merge([upload(h) for h in hosts], comparer=D))
    mergeutil.assert_same(r, merge_host(hosts, comparer=D), "merge, 259 tiles")
    n = 2 * N_RUN
    assert r[0]["n_kv"] == n and (n >> 8) + 1 == 259 and r[0]["status_mask"] == 0
    assert r[1].tolist() == [0, 1] * N_RUN and r[2].tolist() == [i // 2 for i in range(n)]
    assert r[0]["key_off"].tolist() == [6 * i for i in range(n + 1)] and r[0]["val_off"].tolist() == list(range(n + 1))
    assert r[0]["val_bytes"].tolist() == [((i >> 1) + (i & 1)) & 0xff for i in range(n)]


def test_more_than_256_tiles_scan():
    """A 66 200-KV source: the prepare's tile scan takes two steps, and both
    queries begin before tile 256 and end in tile 258, once with every third KV
    of the stretch hidden."""
    n = 2 * N_RUN
    keys = [b"%06d" % i for i in range(n)]
    h = host_from_blocks([[(k, T(7), bytes([i & 0xff])) for i, k in enumerate(keys[:40000])],
                          [(k, T(7), bytes([i & 0xff])) for i, k in enumerate(keys[40000:])]])
    h["kv_flags"][65000:n:3] = N.PBL_KV_OBSOLETE
    d = upload(h)
    lo, up = [keys[255 * 256 + 20], keys[254 * 256 + 200]], [keys[258 * 256 + 52], keys[258 * 256 + 102]]
    for hide in (False, True):
        r = scanutil.device_result(scan(d, lo, up, comparer=D, hide_obsolete_points=hide))
        scanutil.assert_same(r, scan_host(h, lo, up, comparer=D, hide_obsolete_points=hide), ("scan, 259 tiles", hide))
        assert r[1].tolist() == [[255 * 256 + 20, 258 * 256 + 52], [254 * 256 + 200, 258 * 256 + 102]]
        for q in (0, 1):
            a, b = int(r[1][q][0]), int(r[1][q][1])
            src = [i for i in range(a, b) if not (hide and i >= 65000 and (i - 65000) % 3 == 0)]
            kv0 = int(r[0]["blk_kv_base"][q])
            assert r[2][kv0: kv0 + len(src)].tolist() == src and int(r[0]["blk_kv_base"][q + 1]) - kv0 == len(src), (hide, q)
            assert [kv[0] for kv in result_kvs(r[0], q)] == [keys[i] for i in src], (hide, q)


# ---- one call of each operator into a result the test allocated -------------------------------------
def fresh_out(nb, caps, fill, meta=False):
    import torch
    from pebble_amd.batch import Capacity, DecodedBatch
    out = DecodedBatch.allocate(nb, Capacity(caps[0], caps[1], caps[2], 0), "cuda", restarts=False, meta=meta)
    bufs = [out.trailer, out.kv_flags, out.entry_off, out.key_off, out.val_off, out.key_bytes, out.val_bytes]
    if meta:
        bufs += [out.tiering_span_id, out.tiering_attr]
    for x in bufs:
        x.view(torch.uint8).fill_(fill)
    return out, bufs


def src_struct(d, kv_flags=True):
    s = d.c_struct()
    if not kv_flags:
        s.kv_flags = None
    return s


def merge_call(structs, nb, n_kv, out, src_run=None, src_kv=None):
    import torch
    arr = (N.DecodeOutC * len(structs))(*structs)
    rs = N.MergeRunsC(ctypes.cast(arr, ctypes.POINTER(N.DecodeOutC)), len(structs), nb, D, 0, n_kv)
    ws = torch.empty(int(N.lib().pbl_merge_workspace_bytes(len(structs), nb, n_kv)), dtype=torch.uint8, device="cuda")
    mo = N.MergeOutC(out.c_struct(), src_run.data_ptr() if src_run is not None else None,
                     src_kv.data_ptr() if src_kv is not None else None)
    rc = N.lib().pbl_merge_batch(ctypes.byref(rs), ctypes.byref(mo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0, None)
    assert rc == N.PBL_OK
    torch.cuda.synchronize()


def visible_call(struct, nb, n_kv, out, src_kv=None, n_src=None):
    import torch
    vin = N.VisibleInC(struct, nb, D, n_kv, MAX)
    ws = torch.empty(int(N.lib().pbl_visible_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device="cuda")
    vo = N.VisibleOutC(out.c_struct(), src_kv.data_ptr() if src_kv is not None else None,
                       n_src.data_ptr() if n_src is not None else None)
    rc = N.lib().pbl_visible_batch(ctypes.byref(vin), ctypes.byref(vo), ctypes.c_void_p(ws.data_ptr()), ws.numel(), 0, None)
    assert rc == N.PBL_OK
    torch.cuda.synchronize()


def scan_call(d, struct, lo, up, ids, out, src_kv=None):
    import torch
    n = len(lo)
    idx = prepare(d, D, False, n)
    lb, lo_, ub, uo, fl = pack_bounds(lo, up)
    dev = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (lb, lo_, ub, uo, fl)]
    blk = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32)).cuda()
    q = N.ScanQueriesC(*(x.data_ptr() for x in dev), blk.data_ptr(), n, D, 0, 0)
    so = N.ScanOutC(out.c_struct(), None, src_kv.data_ptr() if src_kv is not None else None)
    rc = N.lib().pbl_scan_batch(ctypes.byref(struct), d.n_blocks, idx.n_kv, ctypes.byref(q), ctypes.byref(so),
                                ctypes.c_void_p(idx.workspace.data_ptr()), idx.workspace.numel(), 0, None)
    assert rc == N.PBL_OK
    torch.cuda.synchronize()


# ---- sources without the optional per-KV arrays -----------------------------------------------------
FLAG_CYCLE = [0, N.PBL_KV_RESTART, N.PBL_KV_VALBLK_HANDLE, N.PBL_KV_BLOB_HANDLE | N.PBL_KV_PREFIX_CHANGED,
              N.PBL_KV_RESTART_SAMEPFX | N.PBL_KV_VALBLK_HANDLE, N.PBL_KV_PREFIX_CHANGED]


def plain_source(r=0, flags=True):
    """Three blocks of five KVs, no entry_off, no tiering arrays; kv_flags that
    say nothing to any operator's rules, or none."""
    blocks = [[(b"p%d-%02d" % (q, 2 * j + r), T(9), value(q + j, 3 + j)) for j in range(5)] for q in range(3)]
    h = host_from_blocks(blocks)
    h["kv_flags"] = np.array([FLAG_CYCLE[(i + r) % len(FLAG_CYCLE)] for i in range(15)], np.uint8) if flags else None
    return h


def caps_of(r):
    return (r["n_kv"], r["key_bytes_total"], r["val_bytes_total"])


def meta_is(out, n, byte):
    """entry_off and the tiering arrays of the first n result KVs, as bytes."""
    import torch
    return all(bool((x[:n].view(torch.uint8) == byte).all()) for x in (out.entry_off, out.tiering_span_id, out.tiering_attr))


@pytest.mark.parametrize("flags", [True, False], ids=["kv_flags", "no_kv_flags"])
def test_missing_arrays_merge(flags):
    """A result with entry_off and the tiering arrays from runs without them: zeros."""
    import torch
    hosts = [plain_source(r, flags) for r in (0, 1)]
    exp = merge_host(hosts, comparer=D)
    out, _ = fresh_out(3, caps_of(exp[0]), 0xAA, meta=True)
    sr = torch.empty(30, dtype=torch.uint8, device="cuda")
    sk = torch.empty(30, dtype=torch.int64, device="cuda")
    ds = [upload(dict(h, kv_flags=h["kv_flags"] if flags else np.zeros(15, np.uint8))) for h in hosts]
    merge_call([src_struct(d, flags) for d in ds], 3, 30, out, sr, sk)
    got = out.to_host()
    same_arrays(got, exp[0], ("merge", flags))
    assert got["n_kv"] == 30 and meta_is(out, 30, 0)
    run, at = sr.cpu().numpy(), sk.cpu().numpy()
    assert (run == exp[1]).all() and (at.view(np.uint64) == exp[2]).all()
    want = [int(hosts[r]["kv_flags"][i]) if flags else 0 for r, i in zip(run.tolist(), at.tolist())]
    assert got["kv_flags"].tolist() == want and (any(want) or not flags)


@pytest.mark.parametrize("flags", [True, False], ids=["kv_flags", "no_kv_flags"])
def test_missing_arrays_visible(flags):
    """Zeros as well; of the source's kv_flags only the handle bits come through."""
    import torch
    h = plain_source(0, flags)
    exp = visible_host(h, comparer=D)
    out, _ = fresh_out(3, caps_of(exp[0]), 0xAA, meta=True)
    sk = torch.empty(15, dtype=torch.int64, device="cuda")
    ns = torch.empty(15, dtype=torch.int32, device="cuda")
    d = upload(dict(h, kv_flags=h["kv_flags"] if flags else np.zeros(15, np.uint8)))
    visible_call(src_struct(d, flags), 3, 15, out, sk, ns)
    got = out.to_host()
    same_arrays(got, exp[0], ("visible", flags))
    assert got["n_kv"] == 15 and meta_is(out, 15, 0)
    assert (sk.cpu().numpy().view(np.uint64) == exp[1]).all() and (ns.cpu().numpy().view(np.uint32) == exp[2]).all()
    want = [int(f) & HANDLE_BITS for f in h["kv_flags"]] if flags else [0] * 15
    assert got["kv_flags"].tolist() == want and (len(set(want)) == 3 or not flags)


@pytest.mark.parametrize("flags", [True, False], ids=["kv_flags", "no_kv_flags"])
def test_missing_arrays_scan(flags):
    """The scan leaves the result's entry_off and tiering arrays as they were;
    kv_flags of a source without them are zeros all the same."""
    import torch
    h = plain_source(0, flags)
    lo, up, ids = [None, b"p1-04", None], [None, None, b"p0-06"], [2, 1, 0]
    exp = scan_host(h, lo, up, comparer=D, blocks=ids)
    out, _ = fresh_out(3, caps_of(exp[0]), 0xAA, meta=True)
    sk = torch.empty(15, dtype=torch.int64, device="cuda")
    d = upload(dict(h, kv_flags=h["kv_flags"] if flags else np.zeros(15, np.uint8)))
    scan_call(d, src_struct(d, flags), lo, up, ids, out, sk)
    got = out.to_host()
    same_arrays(got, exp[0], ("scan", flags))
    n = got["n_kv"]
    assert n == 5 + 3 + 3 and meta_is(out, n, 0xAA)
    at = sk.cpu().numpy()[:n]
    assert (at.view(np.uint64) == exp[2]).all()
    want = [int(h["kv_flags"][i]) if flags else 0 for i in at.tolist()]
    assert got["kv_flags"].tolist() == want and (any(want) or not flags)


# ---- a capacity overflow found by the last of three chunks ------------------------------------------
def overflow_check(call, nb, full, extra=()):
    """Each capacity one short in turn: the sizes, the statuses and PBL_OVERFLOW
    come out, and nothing else is written."""
    import torch
    caps = caps_of(full)
    for short in range(3):
        cap = [c - (1 if i == short else 0) for i, c in enumerate(caps)]
        out, bufs = fresh_out(nb, cap, 0xAA)
        side = [torch.full((caps[0],), -1, dtype=dt, device="cuda") for dt in extra]
        call(out, *side)
        t = out.read_totals()
        assert t.status_mask == full["status_mask"] | 1 << N.PBL_OVERFLOW and t.n_bad_blocks == full["n_bad_blocks"], short
        assert (t.n_kv, t.key_bytes, t.val_bytes) == caps, short
        for k in ("blk_kv_base", "blk_key_base", "blk_val_base"):
            assert getattr(out, k).cpu().numpy().view(np.uint64).tolist() == full[k].tolist(), (short, k)
        assert out.blk_status.cpu().numpy().view(np.uint32).tolist() == full["blk_status"].tolist(), short
        for x in bufs:
            assert bool((x.view(torch.uint8) == 0xAA).all()), short
        for x in side:
            assert bool((x == -1).all()), short


def test_overflow_in_the_last_of_three_chunks_merge():
    import torch
    hosts, exp, _ = merge_inputs()
    ds = [upload(h) for h in hosts]
    n_kv = sum(h["n_kv"] for h in hosts)
    overflow_check(lambda out, sr, sk: merge_call([d.c_struct() for d in ds], NB, n_kv, out, sr, sk), NB, exp[0],
                   (torch.int8, torch.int64))


def test_overflow_in_the_last_of_three_chunks_visible():
    import torch
    h, exp, _ = visible_inputs()
    d = upload(h)
    overflow_check(lambda out, sk, ns: visible_call(d.c_struct(), NB, h["n_kv"], out, sk, ns), NB, exp[0],
                   (torch.int64, torch.int32))


def test_overflow_in_the_last_of_three_chunks_scan():
    import torch
    h, (lo, up, ids), exp, _ = scan_inputs()
    d = upload(h)
    overflow_check(lambda out, sk: scan_call(d, d.c_struct(), lo, up, ids, out, sk), NB, exp[0], (torch.int64,))
