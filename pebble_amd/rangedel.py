"""Range deletions in the device read path.

A *run* is one table's range-deletion fragments as a `DecodedBatch` with one
block (key = start, trailer = seq << 8 | 15, value = end): what `decode` makes of
a row-format range-del block, `Table.range_dels()`.  `build_set()` flattens up
to 16 runs into the *set* (pbl_rangedel_set, pebble_amd/csrc/rangedel.hip): the
distinct boundary keys in order, each with the newest tombstone visible at the
snapshot that covers it.  The set is a `DecodedBatch` again, so `to_host()`,
`DataIter` and the per-block seeks read it unchanged.  `cover()` looks every KV
of a batch up in the set (pbl_rangedel_cover): the sequence number of the newest
visible tombstone over its key, which `visible(..., cover=)` takes as one more
invisible predicate per KV.  `build_set_host()` / `cover_host()` run the host
forms over `to_host()` dicts, other algorithms on purpose; `cover_host` takes
the runs, not the set, so it checks the builder and the lookup together.
Levels are optional everywhere (`levels=`, `src_run=` / `run_levels=`): with
them a tombstone of a shallower level deletes whatever the sequence numbers are.
torch is plumbing here: device memory and streams."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from . import _native as N
from .batch import Capacity, DecodedBatch, DecodeError
from .merge import host_struct
from .scan import _n_kv
from .visible import SEQNUM_MAX

MAX_RUNS = N.PBL_RANGEDEL_MAX_RUNS
KIND_RANGEDEL = N.PBL_KIND_RANGEDEL


def _runs_struct(structs, n_kv, comparer: int, snapshot: int, levels=None):
    arr = (N.DecodeOutC * max(len(structs), 1))(*structs)
    cnt = (ctypes.c_uint64 * max(len(structs), 1))(*n_kv)
    lv = None
    if levels is not None:
        if len(levels) != len(structs) or any(not 0 <= int(x) < 255 for x in levels):
            raise ValueError("levels: one in [0, 255) per run")
        lv = (ctypes.c_uint8 * max(len(structs), 1))(*[int(x) for x in levels])
    return (arr, cnt, lv), N.RangedelRunsC(ctypes.cast(arr, ctypes.POINTER(N.DecodeOutC)),
                                           ctypes.cast(cnt, ctypes.POINTER(ctypes.c_uint64)), len(structs), comparer,
                                           snapshot, ctypes.cast(lv, ctypes.POINTER(ctypes.c_uint8)) if lv else None)


def _level_table(run_levels):
    t = [int(x) for x in run_levels]
    if len(t) > MAX_RUNS or any(not 0 <= x < 255 for x in t):
        raise ValueError(f"run_levels: at most {MAX_RUNS} levels in [0, 255)")
    return (ctypes.c_uint8 * MAX_RUNS)(*(t + [0] * (MAX_RUNS - len(t))))


def _bounds(kvs: int, key: int, val: int) -> Capacity:
    """What a set of these runs holds at most: two boundaries per fragment, every start and end byte."""
    return Capacity(kv=2 * kvs, key=key + val, val=0, rst=0)


def build_set(runs: Sequence[DecodedBatch], comparer: int, snapshot: int = SEQNUM_MAX, stream=None,
              levels=None) -> DecodedBatch:
    """The flattened set of the runs for `snapshot`.  `levels` (one per run,
    smaller = shallower): the set also records, per boundary, the shallowest
    level that covers it (entry_off), for `cover(..., src_run=, run_levels=)`.  No size call: the result is
    allocated at its upper bound from the runs' totals.  The set's status is in
    its totals (`read_totals().status_mask`) and `blk_status[0]`; a set with a
    status is empty."""
    runs = list(runs)
    if len(runs) > MAX_RUNS:
        raise ValueError(f"at most {MAX_RUNS} runs")
    if any(r.n_blocks != 1 for r in runs):
        raise ValueError("a run is a decoded batch with one block")
    if not runs:
        raise ValueError("no runs: there is nothing to build a set on (pass cover=None to visible)")
    dev = runs[0].trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    tots = [r._host_totals or r.read_totals() for r in runs]
    n_kv = [int(t.n_kv) for t in tots]
    cap = _bounds(sum(n_kv), sum(int(t.key_bytes) for t in tots), sum(int(t.val_bytes) for t in tots))
    lib = N.lib()
    keep, rs = _runs_struct([r.c_struct() for r in runs], n_kv, comparer, snapshot, levels)
    with torch.cuda.stream(st):
        ws = torch.empty(int(lib.pbl_rangedel_workspace_bytes(sum(n_kv))), dtype=torch.uint8, device=dev)
        out = DecodedBatch.allocate(1, cap, dev, entry_off=levels is not None, restarts=False)
    oc = out.c_struct()
    rc = lib.pbl_rangedel_set(ctypes.byref(rs), ctypes.byref(oc), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                              ctypes.c_void_p(st.cuda_stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangedel_set failed: {N.STATUS_NAMES.get(rc, rc)}")
    st.synchronize()
    out.read_totals()
    del keep
    return out


def cover(set_: DecodedBatch, batch: DecodedBatch, comparer: int, stream=None, src_run=None,
          run_levels=None) -> torch.Tensor:
    """int64 [n_kv]: per KV of `batch` the sequence number of the newest visible
    tombstone of the set over its key, 0 for none.  A set with a status covers
    nothing; its status is the set's to report (`build_set`).  With `src_run`
    (uint8 [n_kv], the run every KV came from: a merge's) and `run_levels` (that
    run's level) over a set built with levels, a KV under a tombstone of a
    shallower level gets PBL_RANGEDEL_ALL whatever the sequence numbers are."""
    if (src_run is None) != (run_levels is None):
        raise ValueError("src_run and run_levels go together")
    dev = batch.trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n_kv = _n_kv(batch)
    with torch.cuda.stream(st):
        out = torch.empty(max(n_kv, 1), dtype=torch.int64, device=dev)
    sc, bc = set_.c_struct(), batch.c_struct()
    if src_run is not None:
        if src_run.dtype != torch.uint8 or src_run.device != dev or src_run.numel() < n_kv or not src_run.is_contiguous():
            raise ValueError("src_run: a contiguous uint8 tensor of n_kv entries on the batch's device")
        if set_.entry_off is None:
            raise ValueError("the set was built without levels")
        tbl = _level_table(run_levels)
        rc = N.lib().pbl_rangedel_cover_lv(ctypes.byref(sc), ctypes.byref(bc), batch.n_blocks, n_kv, comparer,
                                           ctypes.c_void_p(src_run.data_ptr()), tbl, ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(st.cuda_stream))
    else:
        rc = N.lib().pbl_rangedel_cover(ctypes.byref(sc), ctypes.byref(bc), batch.n_blocks, n_kv, comparer,
                                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st.cuda_stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangedel_cover failed: {N.STATUS_NAMES.get(rc, rc)}")
    return out[:n_kv]


def _host_runs(hosts, comparer, snapshot, keep, levels=None):
    structs = [host_struct(h, keep) for h in hosts]
    return _runs_struct(structs, [int(h["n_kv"]) for h in hosts], comparer, snapshot, levels)


def build_set_host(hosts: Sequence[dict], comparer: int, snapshot: int = SEQNUM_MAX, cap: Capacity = None,
                   levels=None) -> dict:
    """The same set over host arrays (`to_host()` dicts of the runs) through
    pbl_rangedel_set_host, as a dict in `to_host()`'s layout.  `cap`: the
    capacities to offer (default: the upper bound)."""
    hosts = list(hosts)
    keep: list = []
    arr, rs = _host_runs(hosts, comparer, snapshot, keep, levels)
    if cap is None:
        cap = _bounds(sum(int(h["n_kv"]) for h in hosts), sum(int(h["key_bytes_total"]) for h in hosts),
                      sum(int(h["val_bytes_total"]) for h in hosts))
    r = {k: np.zeros(2, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
    r["blk_status"] = np.zeros(1, np.uint32)
    arrays = {"trailer": np.zeros(max(cap.kv, 1), np.uint64), "kv_flags": np.zeros(max(cap.kv, 1), np.uint8),
              "key_off": np.zeros(cap.kv + 1, np.uint32), "val_off": np.zeros(cap.kv + 1, np.uint32),
              "key_bytes": np.zeros(max(cap.key, 1), np.uint8), "val_bytes": np.zeros(1, np.uint8)}
    if levels is not None:
        arrays["entry_off"] = np.zeros(max(cap.kv, 1), np.uint32)
    tot = N.TotalsC()
    o = N.DecodeOutC()
    for k, a in {**r, **arrays}.items():
        setattr(o, k, a.ctypes.data)
    o.totals = ctypes.addressof(tot)
    o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
    rc = N.lib().pbl_rangedel_set_host(ctypes.byref(rs), ctypes.byref(o))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangedel_set_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    over = bool(tot.status_mask & (1 << N.PBL_OVERFLOW))
    n, kb = (0, 0) if over else (int(tot.n_kv), int(tot.key_bytes))
    res = {"trailer": arrays["trailer"][:n], "kv_flags": arrays["kv_flags"][:n],
           "entry_off": arrays["entry_off"][:n] if levels is not None else None,
           "key_off": arrays["key_off"][: n + 1], "val_off": arrays["val_off"][: n + 1],
           "key_bytes": arrays["key_bytes"][:kb], "val_bytes": arrays["val_bytes"][:0], "restarts": None, **r}
    res.update(n_kv=int(tot.n_kv), key_bytes_total=int(tot.key_bytes), val_bytes_total=int(tot.val_bytes), n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    del arr, keep
    return res


def cover_host(hosts: Sequence[dict], batch: dict, comparer: int, snapshot: int = SEQNUM_MAX, levels=None,
               src_run=None, run_levels=None):
    """(uint64 [n_kv], status): the brute-force cover of every KV of the host
    batch under the RUNS (pbl_rangedel_cover_host), and the status their set
    has (all zeros with a status)."""
    hosts = list(hosts)
    keep: list = []
    arr, rs = _host_runs(hosts, comparer, snapshot, keep, levels)
    nb = len(batch["blk_status"])
    b = host_struct(batch, keep)
    out = np.zeros(max(int(batch["n_kv"]), 1), np.uint64)
    st = ctypes.c_uint32(0)
    if src_run is not None:
        sr = np.ascontiguousarray(src_run, np.uint8)
        sr = sr if sr.size else np.zeros(1, np.uint8)
        rc = N.lib().pbl_rangedel_cover_host_lv(ctypes.byref(rs), ctypes.byref(b), nb, sr.ctypes.data,
                                                _level_table(run_levels), out.ctypes.data, ctypes.byref(st))
    else:
        rc = N.lib().pbl_rangedel_cover_host(ctypes.byref(rs), ctypes.byref(b), nb, out.ctypes.data, ctypes.byref(st))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangedel_cover_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    del arr, keep
    return out[: int(batch["n_kv"])], int(st.value)
