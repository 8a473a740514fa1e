"""Compaction view of a sorted decoded batch.

`compact()` turns "several tables' KVs in order" into "what a compaction must
keep", inside HBM (pbl_compact_size + pbl_compact_batch,
pebble_amd/csrc/compact.hip): per block what the reference's compact.Iter
returns over the point keys -- one entry per user key per snapshot stripe,
tombstones unless elided, SET -> SETWITHDEL, MERGE chains folded inside a
stripe, SINGLEDEL consuming one SET / MERGE, DELSIZED sizes, zeroed sequence
numbers in the bottommost stripe (include/pebble_amd.h states the rules).  The
result is a `DecodedBatch` again.  `compact_host()` runs the sequential loop
over host arrays (pbl_compact_batch_host), the reference the device path is
tested against.  `compact_tables()` is decode -> scan -> merge -> compact over
several tables, the compaction-side sibling of `read()`;
`compact_tables_to_blocks()` adds the row-block encoder (pebble_amd.rowenc), so
that what the compaction keeps leaves the device as data blocks.  torch is
plumbing here: device memory and streams."""
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


@dataclass
class CompactResult:
    batch: DecodedBatch              # block q = what a compaction of block q keeps
    src_kv: torch.Tensor             # int64 [n_kv]: the input KV that heads every result KV
    n_src: torch.Tensor              # int32 [n_kv]: the operands of a folded MERGE chain, 1 otherwise
    pinned: torch.Tensor             # uint8 [n_kv]: Iter.SnapshotPinned()
    n_missized: torch.Tensor         # int32 [n_blocks]: IterStats.CountMissizedDels
    n_ineffectual: torch.Tensor      # int32 [n_blocks]: calls of IneffectualSingleDeleteCallback
    n_nondeterministic: torch.Tensor  # int32 [n_blocks]: calls of NondeterministicSingleDeleteCallback


def _flags(elide_tombstones: bool, bottommost: bool) -> int:
    return (N.PBL_COMPACT_ELIDE_TOMBSTONES if elide_tombstones else 0) | (N.PBL_COMPACT_BOTTOMMOST if bottommost else 0)


def _snapshots(snapshots) -> np.ndarray:
    """Sorted, as the reference's test does (slices.Sort)."""
    s = np.sort(np.asarray(list(snapshots), dtype=np.uint64))
    return np.ascontiguousarray(s)


def compact(batch: DecodedBatch, *, comparer: int, snapshots=(), elide_tombstones: bool = False,
            bottommost: bool = False, stream=None) -> CompactResult:
    """Sizes first (pbl_compact_size), one read of the totals, exact allocation,
    then the emit with everything the size call left in the workspace
    (PBL_COMPACT_SIZED): the input is classified once."""
    dev = batch.trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    nb, n_kv = batch.n_blocks, _n_kv(batch)
    lib = N.lib()
    snaps = _snapshots(snapshots)
    flags = _flags(elide_tombstones, bottommost)
    h = ctypes.c_void_p(st.cuda_stream)
    with torch.cuda.stream(st):
        sd = torch.from_numpy(snaps.view(np.int64)).to(dev) if snaps.size else None
        ws = torch.empty(int(lib.pbl_compact_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device=dev)
        sized = DecodedBatch.allocate(nb, Capacity(0, 0, 0, 0), dev, entry_off=False, restarts=False)
        counts = torch.zeros((3, max(nb, 1)), dtype=torch.int32, device=dev)
    cin = N.CompactInC(batch.c_struct(), nb, comparer, n_kv, sd.data_ptr() if sd is not None else None, int(snaps.size))
    wp = ctypes.c_void_p(ws.data_ptr())
    so = N.CompactOutC(sized.c_struct(), None, None, None, None, None, None)
    rc = lib.pbl_compact_size(ctypes.byref(cin), ctypes.byref(so), wp, ws.numel(), flags, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_compact_size failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    t = sized.read_totals()
    cap = Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=0)
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(nb, cap, dev, entry_off=batch.entry_off is not None, restarts=False,
                                    meta=batch.tiering_span_id is not None)
        src_kv = torch.empty(max(cap.kv, 1), dtype=torch.int64, device=dev)
        n_src = torch.empty(max(cap.kv, 1), dtype=torch.int32, device=dev)
        pinned = torch.empty(max(cap.kv, 1), dtype=torch.uint8, device=dev)
    oo = N.CompactOutC(out.c_struct(), src_kv.data_ptr(), n_src.data_ptr(), pinned.data_ptr(), counts[0].data_ptr(),
                       counts[1].data_ptr(), counts[2].data_ptr())
    rc = lib.pbl_compact_batch(ctypes.byref(cin), ctypes.byref(oo), wp, ws.numel(), flags | N.PBL_COMPACT_SIZED, h)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_compact_batch failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    out.read_totals()
    return CompactResult(out, src_kv[: cap.kv], n_src[: cap.kv], pinned[: cap.kv], counts[0][:nb], counts[1][:nb],
                         counts[2][:nb])


def compact_host(host: dict, *, comparer: int, snapshots=(), elide_tombstones: bool = False, bottommost: bool = False,
                 sort_snapshots: bool = True):
    """The same view over host arrays (a `DecodedBatch.to_host()` dict) through
    pbl_compact_batch_host: a dict with `batch` (the result in `to_host()`'s
    layout), `src_kv` uint64 [n_kv], `n_src` uint32 [n_kv], `pinned` uint8
    [n_kv], and `n_missized`, `n_ineffectual`, `n_nondeterministic` uint32
    [n_blocks].  `sort_snapshots=False` hands the list over as given (an
    unsorted one is then PBL_INVALID_ARG)."""
    lib = N.lib()
    n = len(host["blk_status"])
    keep: list = []
    snaps = _snapshots(snapshots) if sort_snapshots else np.ascontiguousarray(np.asarray(list(snapshots), np.uint64))
    cin = N.CompactInC(host_struct(host, keep), n, comparer, 0, snaps.ctypes.data if snaps.size else None, int(snaps.size))
    flags = _flags(elide_tombstones, bottommost)
    entry = host.get("entry_off") is not None
    meta = host.get("tiering_span_id") is not None
    r = {k: np.zeros(n + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
    r["blk_status"] = np.zeros(max(n, 1), np.uint32)
    counts = np.zeros((3, max(n, 1)), np.uint32)
    tot = N.TotalsC()

    def run(cap: Capacity, arrays: dict, per_kv):
        o = N.DecodeOutC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
        co = N.CompactOutC(o, *[a.ctypes.data if a is not None else None for a in per_kv], counts[0].ctypes.data,
                           counts[1].ctypes.data, counts[2].ctypes.data)
        rc = lib.pbl_compact_batch_host(ctypes.byref(cin), ctypes.byref(co), flags)
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_compact_batch_host failed: {N.STATUS_NAMES.get(rc, rc)}")

    run(Capacity(0, 0, 0, 0), {}, (None, None, None))  # sizes (an overflow writes nothing else)
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
    pinned = np.zeros(max(cap.kv, 1), np.uint8)
    run(cap, arrays, (src_kv, n_src, pinned))
    res = {k: a[: cap.kv] for k, a in arrays.items() if k not in ("key_off", "val_off", "key_bytes", "val_bytes")}
    res.update(key_off=arrays["key_off"][: cap.kv + n], val_off=arrays["val_off"][: cap.kv + n],
               key_bytes=arrays["key_bytes"][: cap.key], val_bytes=arrays["val_bytes"][: cap.val],
               entry_off=res.get("entry_off"), restarts=None, **r)
    res["blk_status"] = r["blk_status"][:n]
    res.update(n_kv=cap.kv, key_bytes_total=cap.key, val_bytes_total=cap.val, n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    del keep
    return {"batch": res, "src_kv": src_kv[: cap.kv], "n_src": n_src[: cap.kv], "pinned": pinned[: cap.kv],
            "n_missized": counts[0][:n], "n_ineffectual": counts[1][:n], "n_nondeterministic": counts[2][:n]}


def compact_tables(tables, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], *, snapshots=(),
                   elide_tombstones: bool = False, bottommost: bool = False) -> CompactResult:
    """`merge_scan` of the tables over the ranges, then `compact`: per range what
    compact.NewIter over the tables' point keys returns (src_kv indexes the merge
    result).  Range deletions and range keys are not part of this view: a table
    that holds either is refused, not read without them."""
    tables = list(tables)
    for t in tables:
        if hasattr(t, "range_dels") and t.range_dels() is not None:
            raise ValueError("compact_tables: a table holds range deletions, which the compaction view does not apply")
        if hasattr(t, "range_keys") and t.range_keys() is not None:
            raise ValueError("compact_tables: a table holds range keys, which the compaction view does not carry")
    comparer = tables[0].comparer()
    merged = merge_scan(tables, lowers, uppers)
    return compact(merged.batch, comparer=comparer, snapshots=snapshots, elide_tombstones=elide_tombstones,
                   bottommost=bottommost)


def compact_tables_to_blocks(tables, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], opts, *,
                             snapshots=(), elide_tombstones: bool = False, bottommost: bool = False):
    """`compact_tables`, then `rowenc.encode` of what it keeps: every range is
    one stream, written as a fresh table writer with `opts` (a `RowEncOptions`;
    its comparer must be the tables') would write it.  Returns (CompactResult,
    EncodedBlocks): block b holds the result KVs block_first_kv[b] .. +
    block_n_kv[b] of range block_stream[b]."""
    from .rowenc import encode
    tables = list(tables)
    if opts.comparer != tables[0].comparer():
        raise ValueError("compact_tables_to_blocks: the options' comparer is not the tables'")
    res = compact_tables(tables, lowers, uppers, snapshots=snapshots, elide_tombstones=elide_tombstones,
                         bottommost=bottommost)
    return res, encode(res.batch, opts)
