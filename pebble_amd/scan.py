"""Batched bounded scans over a decoded batch.

`scan()` takes the KVs of many key ranges [lower, upper) out of a
`DecodedBatch` in HBM (pbl_scan_size + pbl_scan_batch, pebble_amd/csrc/scan.hip):
per query, exactly what singleLevelIterator returns for SetBounds(lower, upper);
First(); Next()... (include/pebble_amd.h states both modes).  The result is a
`DecodedBatch` with one "block" per query, so `to_host()`, `DataIter` and the
per-block seeks read it unchanged.  `prepare()` builds the seek fence and the
visible prefix once (pbl_scan_prepare); `scan_host()` runs the same bounds
search and a plain gather over host arrays (pbl_scan_batch_host), the reference
the device path is tested against.  torch is plumbing here: device memory and
streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N
from .batch import Capacity, DecodedBatch, DecodeError, _stream_handle
from .seek import pack_keys

Bound = Union[Sequence[Optional[bytes]], Tuple[torch.Tensor, torch.Tensor]]


@dataclass
class ScanIndex:
    """The seek fence and the visible prefix of one decoded batch under one
    comparer and one hide flag.  Its workspace also holds the per-query state of
    the scan in flight: one scan at a time per index."""
    workspace: torch.Tensor  # uint8, device
    comparer: int
    hide_obsolete_points: bool
    n_blocks: int
    n_kv: int
    n_queries: int           # the most queries one scan over this workspace may hold


@dataclass
class ScanResult:
    batch: DecodedBatch   # one "block" per query
    range: torch.Tensor   # int64 [n, 2]: source KV index range [kv_lo, kv_hi) before hiding
    src_kv: torch.Tensor  # int64 [n_kv]: source KV index of every result KV


def _n_kv(decoded: DecodedBatch) -> int:
    t = decoded._host_totals if decoded._host_totals is not None else decoded.read_totals()
    return int(t.n_kv)


def prepare(decoded: DecodedBatch, comparer: int, hide_obsolete_points: bool = False, n_queries: int = 1024,
            stream=None) -> ScanIndex:
    lib = N.lib()
    nb, nkv = decoded.n_blocks, _n_kv(decoded)
    ws = torch.empty(int(lib.pbl_scan_workspace_bytes(n_queries, nb, nkv)), dtype=torch.uint8,
                     device=decoded.trailer.device)
    o = decoded.c_struct()
    rc = lib.pbl_scan_prepare(ctypes.byref(o), nb, nkv, comparer, 1 if hide_obsolete_points else 0,
                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream_handle(stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_scan_prepare failed: {N.STATUS_NAMES.get(rc, rc)}")
    return ScanIndex(ws, comparer, bool(hide_obsolete_points), nb, nkv, n_queries)


def pack_bounds(lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]]):
    """(lower bytes, lower offsets, upper bytes, upper offsets, flags) as numpy:
    a None lower is the empty key (First()), a None upper PBL_SCAN_NO_UPPER."""
    if len(lowers) != len(uppers):
        raise ValueError("one upper bound per lower bound")
    lb, lo = pack_keys([k or b"" for k in lowers])
    ub, uo = pack_keys([k or b"" for k in uppers])
    fl = np.array([N.PBL_SCAN_NO_UPPER if k is None else 0 for k in uppers], np.uint8)
    return lb, lo, ub, uo, fl


def _result_struct(batch: DecodedBatch, rng, src) -> N.ScanOutC:
    return N.ScanOutC(batch.c_struct(), rng, src)


def scan(decoded: DecodedBatch, lowers: Bound, uppers: Bound, *, comparer: int, blocks=None,
         hide_obsolete_points: bool = False, index: Optional[ScanIndex] = None, flags=None,
         stream=None) -> ScanResult:
    """Scan every range.  Bounds: lists of bytes (None = unbounded), or (uint8
    tensor readable 16 B past the last key, int64 offsets [n + 1]) already on
    the device, with `flags` (uint8 [n], PBL_SCAN_NO_UPPER) for the upper ones.
    `blocks` (a sequence or an int32 device tensor, one block id per query)
    selects per-block mode.  Sizes first (pbl_scan_size), one read of the
    totals, exact allocation, then the emit with the bounds the size call left
    in the workspace (PBL_SCAN_SIZED): the searches run once."""
    dev = decoded.trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    if isinstance(lowers, tuple):
        (lb, lo), (ub, uo) = lowers, uppers
        fl = flags
    else:
        hlb, hlo, hub, huo, hfl = pack_bounds(list(lowers), list(uppers))
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        lb, lo, ub, uo, fl = up(hlb), up(hlo.view(np.int64)), up(hub), up(huo.view(np.int64)), up(hfl)
    n = int(lo.numel()) - 1
    if int(uo.numel()) - 1 != n:
        raise ValueError("one upper bound per lower bound")
    blk = None
    if blocks is not None:
        blk = blocks if isinstance(blocks, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.uint32).view(np.int32)).to(dev)
        if int(blk.numel()) != n:
            raise ValueError("one block id per query")
    if index is None or index.n_queries < n:
        index = prepare(decoded, comparer, hide_obsolete_points, max(n, 1), st)
    if (index.n_blocks != decoded.n_blocks or index.hide_obsolete_points != bool(hide_obsolete_points) or
            (blk is None and index.comparer != comparer)):
        raise ValueError("the ScanIndex was prepared for another comparer, hide flag or batch")
    lib = N.lib()
    q = N.ScanQueriesC(lb.data_ptr(), lo.data_ptr(), ub.data_ptr(), uo.data_ptr(),
                       fl.data_ptr() if fl is not None else None, blk.data_ptr() if blk is not None else None, n,
                       comparer, 1 if hide_obsolete_points else 0, 0)
    src = decoded.c_struct()
    ws = ctypes.c_void_p(index.workspace.data_ptr())
    h = ctypes.c_void_p(st.cuda_stream)
    with torch.cuda.stream(st):
        rng = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev)
        sized = DecodedBatch.allocate(n, Capacity(0, 0, 0, 0), dev, entry_off=False, restarts=False)
    so = _result_struct(sized, rng.data_ptr(), None)
    rc = lib.pbl_scan_size(ctypes.byref(src), decoded.n_blocks, index.n_kv, ctypes.byref(q), ctypes.byref(so), ws,
                           index.workspace.numel(), h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_scan_size failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    t = sized.read_totals()
    cap = Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=0)
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(n, cap, dev, entry_off=decoded.entry_off is not None, restarts=False,
                                    meta=decoded.tiering_span_id is not None)
        src_kv = torch.empty(max(cap.kv, 1), dtype=torch.int64, device=dev)
    oo = _result_struct(out, rng.data_ptr(), src_kv.data_ptr())
    rc = lib.pbl_scan_batch(ctypes.byref(src), decoded.n_blocks, index.n_kv, ctypes.byref(q), ctypes.byref(oo), ws,
                            index.workspace.numel(), N.PBL_SCAN_SIZED, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_scan_batch failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    out.read_totals()
    return ScanResult(out, rng[:n], src_kv[: cap.kv])


_HOST_IN = ("trailer", "kv_flags", "entry_off", "key_off", "val_off", "key_bytes", "val_bytes", "blk_kv_base",
            "blk_key_base", "blk_val_base", "blk_status", "tiering_span_id", "tiering_attr")


def scan_host(host: dict, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], *, comparer: int,
              blocks=None, hide_obsolete_points: bool = False):
    """The same scan over host arrays (`DecodedBatch.to_host()` or the oracle's
    dict) through pbl_scan_batch_host: (result dict in `to_host()`'s layout,
    range uint64 [n, 2], src_kv uint64 [n_kv])."""
    lib = N.lib()
    nb = len(host["blk_status"])
    keep = {}
    d = N.DecodeOutC()
    for k in _HOST_IN:
        a = host.get(k)
        if a is None:
            continue
        a = np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))
        keep[k] = a
        setattr(d, k, a.ctypes.data)
    lb, lo, ub, uo, fl = pack_bounds(list(lowers), list(uppers))
    n = len(lo) - 1
    blk = np.ascontiguousarray(blocks, dtype=np.uint32) if blocks is not None else None
    q = N.ScanQueriesC(lb.ctypes.data, lo.ctypes.data, ub.ctypes.data, uo.ctypes.data, fl.ctypes.data if n else None,
                       blk.ctypes.data if blk is not None else None, n, comparer, 1 if hide_obsolete_points else 0, 0)
    meta = "tiering_span_id" in keep
    r = {k: np.zeros(n + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
    r["blk_status"] = np.zeros(max(n, 1), np.uint32)
    rng = np.zeros((max(n, 1), 2), np.uint64)
    tot = N.TotalsC()

    def run(cap: Capacity, arrays: dict, src):
        o = N.DecodeOutC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
        so = N.ScanOutC(o, rng.ctypes.data, src.ctypes.data if src is not None else None)
        rc = lib.pbl_scan_batch_host(ctypes.byref(d), nb, ctypes.byref(q), ctypes.byref(so))
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_scan_batch_host failed: {N.STATUS_NAMES.get(rc, rc)}")

    run(Capacity(0, 0, 0, 0), {}, None)  # sizes (an overflow writes nothing else)
    cap = Capacity(int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes), 0)
    arrays = {"trailer": np.zeros(max(cap.kv, 1), np.uint64), "kv_flags": np.zeros(max(cap.kv, 1), np.uint8),
              "key_off": np.zeros(cap.kv + n + 1, np.uint32), "val_off": np.zeros(cap.kv + n + 1, np.uint32),
              "key_bytes": np.zeros(max(cap.key, 1), np.uint8), "val_bytes": np.zeros(max(cap.val, 1), np.uint8)}
    if "entry_off" in keep:
        arrays["entry_off"] = np.zeros(max(cap.kv, 1), np.uint32)
    if meta:
        arrays["tiering_span_id"] = np.zeros(max(cap.kv, 1), np.uint64)
        arrays["tiering_attr"] = np.zeros(max(cap.kv, 1), np.uint64)
    src = np.zeros(max(cap.kv, 1), np.uint64)
    run(cap, arrays, src)
    res = {k: a[: cap.kv] for k, a in arrays.items() if k not in ("key_off", "val_off", "key_bytes", "val_bytes")}
    res.update(key_off=arrays["key_off"][: cap.kv + n], val_off=arrays["val_off"][: cap.kv + n],
               key_bytes=arrays["key_bytes"][: cap.key], val_bytes=arrays["val_bytes"][: cap.val],
               entry_off=res.get("entry_off"), restarts=None, **r)
    res["blk_status"] = r["blk_status"][:n]
    res.update(n_kv=cap.kv, key_bytes_total=cap.key, val_bytes_total=cap.val, n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    return res, rng[:n], src[: cap.kv]
