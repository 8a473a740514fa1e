"""Batched k-way merge of sorted decoded batches.

`merge()` interleaves K `DecodedBatch`es with the same number of blocks inside
HBM (pbl_merge_size + pbl_merge_batch, pebble_amd/csrc/merge.hip): result block
q is the sequence mergingIter.First(); Next()... yields over block q of every
run (user key ascending under the comparer, trailer descending, equal internal
keys in run order; include/pebble_amd.h states the semantics).  The result is a
`DecodedBatch` again, so `to_host()`, `DataIter`, the per-block seeks, `scan()`
and `merge()` read it unchanged.  `merge_host()` runs a plain k-way merge over
host arrays (pbl_merge_batch_host), the reference the device path is tested
against.  `merge_scan()` is decode -> scan -> merge over several tables.  torch
is plumbing here: device memory and streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .batch import Capacity, DecodedBatch, DecodeError
from .scan import _HOST_IN, _n_kv


@dataclass
class MergeResult:
    batch: DecodedBatch    # block q = the merge of block q of every run
    src_run: torch.Tensor  # uint8 [n_kv]: the run of every result KV
    src_kv: torch.Tensor   # int64 [n_kv]: its KV index in that run


def _runs_struct(structs, n_blocks: int, comparer: int, n_kv_total: int):
    arr = (N.DecodeOutC * max(len(structs), 1))(*structs)
    return arr, N.MergeRunsC(ctypes.cast(arr, ctypes.POINTER(N.DecodeOutC)), len(structs), n_blocks, comparer, 0,
                             n_kv_total)


def merge(runs: Sequence[DecodedBatch], *, comparer: int, stream=None) -> MergeResult:
    """Merge block q of every run, for every q.  Sizes first (pbl_merge_size),
    one read of the totals, exact allocation, then the emit with the statuses
    and sizes the size call left in the workspace (PBL_MERGE_SIZED): the runs
    are validated once."""
    runs = list(runs)
    if not 1 <= len(runs) <= N.PBL_MERGE_MAX_RUNS:
        raise ValueError(f"1 to {N.PBL_MERGE_MAX_RUNS} runs")
    nb = runs[0].n_blocks
    if any(r.n_blocks != nb for r in runs):
        raise ValueError("every run needs the same number of blocks")
    dev = runs[0].trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n_kv = sum(_n_kv(r) for r in runs)
    lib = N.lib()
    keep, rs = _runs_struct([r.c_struct() for r in runs], nb, comparer, n_kv)
    h = ctypes.c_void_p(st.cuda_stream)
    with torch.cuda.stream(st):
        ws = torch.empty(int(lib.pbl_merge_workspace_bytes(len(runs), nb, n_kv)), dtype=torch.uint8, device=dev)
        sized = DecodedBatch.allocate(nb, Capacity(0, 0, 0, 0), dev, entry_off=False, restarts=False)
    wp = ctypes.c_void_p(ws.data_ptr())
    so = N.MergeOutC(sized.c_struct(), None, None)
    rc = lib.pbl_merge_size(ctypes.byref(rs), ctypes.byref(so), wp, ws.numel(), h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_merge_size failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    t = sized.read_totals()
    cap = Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=0)
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(nb, cap, dev, entry_off=all(r.entry_off is not None for r in runs),
                                    restarts=False, meta=any(r.tiering_span_id is not None for r in runs))
        src_run = torch.empty(max(cap.kv, 1), dtype=torch.uint8, device=dev)
        src_kv = torch.empty(max(cap.kv, 1), dtype=torch.int64, device=dev)
    oo = N.MergeOutC(out.c_struct(), src_run.data_ptr(), src_kv.data_ptr())
    rc = lib.pbl_merge_batch(ctypes.byref(rs), ctypes.byref(oo), wp, ws.numel(), N.PBL_MERGE_SIZED, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_merge_batch failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    out.read_totals()
    del keep
    return MergeResult(out, src_run[: cap.kv], src_kv[: cap.kv])


def host_struct(host: dict, keep: list) -> N.DecodeOutC:
    """pbl_decode_out over the arrays of a `to_host()` dict (`keep` holds them alive)."""
    d = N.DecodeOutC()
    for k in _HOST_IN:
        a = host.get(k)
        if a is None:
            continue
        a = np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))
        keep.append(a)
        setattr(d, k, a.ctypes.data)
    return d


def merge_host(hosts: Sequence[dict], *, comparer: int):
    """The same merge over host arrays (`DecodedBatch.to_host()` dicts) through
    pbl_merge_batch_host: (result dict in `to_host()`'s layout, src_run uint8
    [n_kv], src_kv uint64 [n_kv])."""
    lib = N.lib()
    hosts = list(hosts)
    n = len(hosts[0]["blk_status"]) if hosts else 0
    keep: list = []
    arr, rs = _runs_struct([host_struct(h, keep) for h in hosts], n, comparer, 0)
    entry = bool(hosts) and all(h.get("entry_off") is not None for h in hosts)
    meta = any(h.get("tiering_span_id") is not None for h in hosts)
    r = {k: np.zeros(n + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
    r["blk_status"] = np.zeros(max(n, 1), np.uint32)
    tot = N.TotalsC()

    def run(cap: Capacity, arrays: dict, src_run, src_kv):
        o = N.DecodeOutC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
        mo = N.MergeOutC(o, src_run.ctypes.data if src_run is not None else None,
                         src_kv.ctypes.data if src_kv is not None else None)
        rc = lib.pbl_merge_batch_host(ctypes.byref(rs), ctypes.byref(mo))
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_merge_batch_host failed: {N.STATUS_NAMES.get(rc, rc)}")

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
    src_run = np.zeros(max(cap.kv, 1), np.uint8)
    src_kv = np.zeros(max(cap.kv, 1), np.uint64)
    run(cap, arrays, src_run, src_kv)
    res = {k: a[: cap.kv] for k, a in arrays.items() if k not in ("key_off", "val_off", "key_bytes", "val_bytes")}
    res.update(key_off=arrays["key_off"][: cap.kv + n], val_off=arrays["val_off"][: cap.kv + n],
               key_bytes=arrays["key_bytes"][: cap.key], val_bytes=arrays["val_bytes"][: cap.val],
               entry_off=res.get("entry_off"), restarts=None, **r)
    res["blk_status"] = r["blk_status"][:n]
    res.update(n_kv=cap.kv, key_bytes_total=cap.key, val_bytes_total=cap.val, n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    del arr
    return res, src_run[: cap.kv], src_kv[: cap.kv]


def merge_scan(tables, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], *,
               hide_obsolete_points: bool = False) -> MergeResult:
    """`Table.scan` of every table with the same ranges, then `merge`: per range
    the merged KVs of all tables (src_run = the table, src_kv = the KV index in
    that table's scan result).  One unbounded range merges whole tables; a
    caller cuts larger inputs into ranges under 4 GiB, which is also how the
    work spreads."""
    tables = list(tables)
    cmps = {t.comparer() for t in tables}
    if len(cmps) != 1:
        raise ValueError(f"the tables' comparers differ: {sorted(cmps)}")
    runs = [t.scan(lowers, uppers, hide_obsolete_points=hide_obsolete_points).batch for t in tables]
    return merge(runs, comparer=cmps.pop())
