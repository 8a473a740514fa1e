"""Batched snapshot-visible view of a sorted decoded batch.

`visible()` turns "several tables' KVs in order" into "what a reader sees",
inside HBM (pbl_visible_size + pbl_visible_batch, pebble_amd/csrc/visible.hip):
per block the newest version of every user key below the snapshot, deleted keys
dropped, MERGE chains folded oldest first (include/pebble_amd.h states the
rules).  The result is a `DecodedBatch` again, so `to_host()`, `DataIter`, the
per-block seeks, `scan()` and `merge()` read it unchanged.  `visible_host()`
runs the sequential state machine over host arrays (pbl_visible_batch_host),
the reference the device path is tested against.  `read()` is decode -> scan ->
merge -> visible over several tables: the device-resident equivalent of an
Iterator with bounds.  torch is plumbing here: device memory and streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .batch import Capacity, DecodedBatch, DecodeError
from .merge import host_struct, merge_scan
from .scan import _n_kv

SEQNUM_MAX = N.PBL_SEQNUM_MAX


@dataclass
class VisibleResult:
    batch: DecodedBatch    # block q = what a reader of block q sees
    src_kv: torch.Tensor   # int64 [n_kv]: the input KV every result KV came from
    n_src: torch.Tensor    # int32 [n_kv]: the input KVs whose bytes its value holds


def visible(batch: DecodedBatch, *, comparer: int, snapshot: int = SEQNUM_MAX, keep_operands: bool = False,
            stream=None, cover: Optional[torch.Tensor] = None) -> VisibleResult:
    """Sizes first (pbl_visible_size), one read of the totals, exact allocation,
    then the emit with the statuses, sizes and roles the size call left in the
    workspace (PBL_VISIBLE_SIZED): the input is classified once.  `cover`
    (`rangedel.cover`, int64 [n_kv]): a KV under a newer range tombstone is
    invisible too (the _rd entry points); None is the call sequence without
    range deletions."""
    dev = batch.trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    nb, n_kv = batch.n_blocks, _n_kv(batch)
    lib = N.lib()
    if cover is not None:
        if cover.dtype != torch.int64 or cover.device != dev or cover.numel() < n_kv or not cover.is_contiguous():
            raise ValueError("cover: a contiguous int64 tensor of n_kv entries on the batch's device")
        cp = ctypes.c_void_p(cover.data_ptr())
        size_fn = lambda *a: lib.pbl_visible_size_rd(*a[:5], cp, a[5])  # noqa: E731
        batch_fn = lambda *a: lib.pbl_visible_batch_rd(*a[:5], cp, a[5])  # noqa: E731
    else:
        size_fn, batch_fn = lib.pbl_visible_size, lib.pbl_visible_batch
    vin = N.VisibleInC(batch.c_struct(), nb, comparer, n_kv, snapshot)
    flags = N.PBL_VISIBLE_KEEP_OPERANDS if keep_operands else 0
    h = ctypes.c_void_p(st.cuda_stream)
    with torch.cuda.stream(st):
        ws = torch.empty(int(lib.pbl_visible_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device=dev)
        sized = DecodedBatch.allocate(nb, Capacity(0, 0, 0, 0), dev, entry_off=False, restarts=False)
    wp = ctypes.c_void_p(ws.data_ptr())
    so = N.VisibleOutC(sized.c_struct(), None, None)
    rc = size_fn(ctypes.byref(vin), ctypes.byref(so), wp, ws.numel(), flags, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_visible_size failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    t = sized.read_totals()
    cap = Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=0)
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(nb, cap, dev, entry_off=batch.entry_off is not None, restarts=False,
                                    meta=batch.tiering_span_id is not None)
        src_kv = torch.empty(max(cap.kv, 1), dtype=torch.int64, device=dev)
        n_src = torch.empty(max(cap.kv, 1), dtype=torch.int32, device=dev)
    oo = N.VisibleOutC(out.c_struct(), src_kv.data_ptr(), n_src.data_ptr())
    rc = batch_fn(ctypes.byref(vin), ctypes.byref(oo), wp, ws.numel(), flags | N.PBL_VISIBLE_SIZED, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_visible_batch failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    out.read_totals()
    return VisibleResult(out, src_kv[: cap.kv], n_src[: cap.kv])


def visible_host(host: dict, *, comparer: int, snapshot: int = SEQNUM_MAX, keep_operands: bool = False, cover=None):
    """The same view over host arrays (a `DecodedBatch.to_host()` dict) through
    pbl_visible_batch_host: (result dict in `to_host()`'s layout, src_kv uint64
    [n_kv], n_src uint32 [n_kv]).  `cover` (`rangedel.cover_host`, uint64
    [n_kv]): through pbl_visible_batch_host_rd."""
    lib = N.lib()
    if cover is not None:
        cover = np.ascontiguousarray(cover, np.uint64)
        if cover.size < int(host["n_kv"]):
            raise ValueError("cover: n_kv entries")
        cover = cover if cover.size else np.zeros(1, np.uint64)
    n = len(host["blk_status"])
    keep: list = []
    vin = N.VisibleInC(host_struct(host, keep), n, comparer, 0, snapshot)
    flags = N.PBL_VISIBLE_KEEP_OPERANDS if keep_operands else 0
    entry = host.get("entry_off") is not None
    meta = host.get("tiering_span_id") is not None
    r = {k: np.zeros(n + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
    r["blk_status"] = np.zeros(max(n, 1), np.uint32)
    tot = N.TotalsC()

    def run(cap: Capacity, arrays: dict, src_kv, n_src):
        o = N.DecodeOutC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
        vo = N.VisibleOutC(o, src_kv.ctypes.data if src_kv is not None else None,
                           n_src.ctypes.data if n_src is not None else None)
        if cover is not None:
            rc = lib.pbl_visible_batch_host_rd(ctypes.byref(vin), ctypes.byref(vo), flags, cover.ctypes.data)
        else:
            rc = lib.pbl_visible_batch_host(ctypes.byref(vin), ctypes.byref(vo), flags)
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_visible_batch_host failed: {N.STATUS_NAMES.get(rc, rc)}")

    run(Capacity(0, 0, 0, 0), {}, None, None)  # sizes (an overflow writes nothing else)
    cap = Capacity(int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes), 0)
    arrays = {"trailer": np.zeros(max(cap.kv, 1), np.uint64), "kv_flags": np.zeros(max(cap.kv, 1), np.uint8),
              "key_off": np.zeros(cap.kv + n + 1, np.uint32), "val_off": np.zeros(cap.kv + n + 1, np.uint32),
              "key_bytes": np.zeros(max(cap.key, 1), np.uint8), "val_bytes": np.zeros(max(cap.val, 1), np.uint8)}
    if entry:
        arrays["entry_off"] = np.zeros(max(cap.kv, 1), np.uint32)
    if meta:
        arrays["tiering_span_id"] = np.zeros(max(cap.kv, 1), np.uint64)
        arrays["tiering_attr"] = np.zeros(max(cap.kv, 1), np.uint64)
    src_kv = np.zeros(max(cap.kv, 1), np.uint64)
    n_src = np.zeros(max(cap.kv, 1), np.uint32)
    run(cap, arrays, src_kv, n_src)
    res = {k: a[: cap.kv] for k, a in arrays.items() if k not in ("key_off", "val_off", "key_bytes", "val_bytes")}
    res.update(key_off=arrays["key_off"][: cap.kv + n], val_off=arrays["val_off"][: cap.kv + n],
               key_bytes=arrays["key_bytes"][: cap.key], val_bytes=arrays["val_bytes"][: cap.val],
               entry_off=res.get("entry_off"), restarts=None, **r)
    res["blk_status"] = r["blk_status"][:n]
    res.update(n_kv=cap.kv, key_bytes_total=cap.key, val_bytes_total=cap.val, n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    del keep
    return res, src_kv[: cap.kv], n_src[: cap.kv]


def read(tables, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], *, snapshot: int = SEQNUM_MAX,
         hide_obsolete_points: bool = False, keep_operands: bool = False, range_dels=None, levels=None,
         range_del_levels=None, range_keys=None, with_range_keys: bool = False, mask_suffix: Optional[bytes] = None):
    """`merge_scan` of the tables over the ranges, then `visible`: per range
    what an Iterator with those bounds over the tables returns going forward
    (point keys; src_kv indexes the merge result).  Range deletions apply:
    `range_dels` is a list of runs (`rangedel.build_set`), by default the
    tables' own (`Table.range_dels()`); a caller passes its own for tombstones
    that live elsewhere, for example a memtable's, fragmented by the caller.
    With no tombstones the call sequence is the one without range deletions.
    `levels` (one per table, smaller = shallower) applies the rule level by
    level, as the reference does: a tombstone of a shallower level deletes
    whatever the sequence numbers are.  It matters only where sequence numbers
    are not ordered by level; without it the rule is the sequence-number one.
    Caller-supplied runs then need `range_del_levels`, one per run.

    Range keys (`pebble_amd.rangekey`): `range_keys` is a list of range-key runs
    (`keyspan.Decoded`), by default the tables' own (`Table.range_keys()`).  With
    `with_range_keys` the result is `(points, range_key_batch)`, the second being
    the coalesced, defragmented set at the snapshot truncated to the same ranges
    (`rangekey.clip_host`, on the device as a `keyspan.Decoded` with one block
    per range): what Iterator.RangeBounds / RangeKeys report.  With `mask_suffix`
    (IterOptions.RangeKeyMasking.Suffix) the points that the set masks are
    hidden: `rangekey.mask` stores them into the cover before the view.  The set
    is built by the host form (small next to the batch) and copied over; the
    mask runs on the device.  With none of the three the call path and the
    result are the ones without range keys."""
    tables = list(tables)
    comparer = tables[0].comparer()
    merged = merge_scan(tables, lowers, uppers, hide_obsolete_points=hide_obsolete_points)
    if levels is not None and len(levels) != len(tables):
        raise ValueError("levels: one per table")
    if range_dels is None:
        # (anything with comparer() and scan() serves as a table; one without range_dels() has none)
        own = [(t.range_dels(), i) for i, t in enumerate(tables) if hasattr(t, "range_dels")]
        range_dels = [r for r, _ in own if r is not None]
        range_del_levels = [levels[i] for r, i in own if r is not None] if levels is not None else None
    range_dels = list(range_dels)
    if range_dels and (levels is None) != (range_del_levels is None):
        raise ValueError("levels and range_del_levels go together")
    cover = None
    if range_dels:
        from . import rangedel
        rset = rangedel.build_set(range_dels, comparer, snapshot, levels=range_del_levels)
        mask = int(rset.read_totals().status_mask)
        if mask:
            raise DecodeError("range deletions: " + ", ".join(N.STATUS_NAMES.get(b, str(b)) for b in range(32)
                                                              if mask >> b & 1))
        cover = rangedel.cover(rset, merged.batch, comparer, src_run=merged.src_run if levels is not None else None,
                               run_levels=levels)
    rk_batch = None
    if range_keys is not None or with_range_keys or mask_suffix is not None:
        from . import rangekey
        if range_keys is None:
            own_rk = [t.range_keys() for t in tables if hasattr(t, "range_keys")]
            range_keys = [r for r in own_rk if r is not None]
        hosts = [r.to_host() for r in range_keys]
        rk_set = rangekey.build_set_host(hosts, comparer, snapshot)
        if rk_set["status_mask"]:
            raise DecodeError("range keys: " + ", ".join(N.STATUS_NAMES.get(b, str(b)) for b in range(32)
                                                         if rk_set["status_mask"] >> b & 1))
        dev = merged.batch.trailer.device
        if with_range_keys:
            rk_batch = rangekey.to_device(rangekey.clip_host(rk_set, lowers, uppers, comparer), dev)
        if mask_suffix is not None and rk_set["n_kv"]:
            cover = rangekey.mask(rangekey.to_device(rk_set, dev), merged.batch, comparer, mask_suffix, cover=cover)
    points = visible(merged.batch, comparer=comparer, snapshot=snapshot, keep_operands=keep_operands, cover=cover)
    return (points, rk_batch) if with_range_keys else points
