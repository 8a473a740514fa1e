"""Range keys in the device read path.

A range-key *run* is one table's range-key fragments as
`keyspan.decode(extras=True)` makes them of a `pebble.range_key` block: key =
start, value = end, trailer kind in {19, 20, 21}, and per KV the keyspan.Key's
suffix and value.  The *set* is what a reader of up to 16 such runs sees at a
snapshot: coalesced (rangekey.CoalesceInto, sets only, suffix order) and
defragmented spans, one KV per (span, surviving set), again a decoded batch
with extras (`keyspan.Decoded`), so `to_host()`, `DataIter` and the per-block
seeks read it unchanged; `extras.span[kv]` is the index of the span's first KV.

`mask()` is the device hot path (pbl_rangekey_mask, pebble_amd/csrc/rangekey.hip):
it stores PBL_RANGEDEL_ALL into a cover for every KV of a batch that the set
masks at a threshold suffix; `visible(..., cover=)` then hides those KVs as it
hides range-deleted ones, and a cover from `rangedel.cover()` composes with it.

The set itself and its truncation to ranges are built by host forms
(`build_set_host`, `clip_host`: the reference's sequential shape) and copied to
the device with `to_device()`; a device builder is not built.
`mask_set_host` is the lookup over host arrays; `mask_host` takes the runs, not
the set, and brute-forces every KV, so it checks builder and lookup together.
torch is plumbing here: device memory and streams."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .batch import Capacity, DecodedBatch, DecodeError
from .keyspan import EXTRA_KEYS, Decoded, Extras
from .merge import host_struct
from .scan import _n_kv
from .visible import SEQNUM_MAX

MAX_RUNS = N.PBL_RANGEDEL_MAX_RUNS
KIND_DEL, KIND_UNSET, KIND_SET = N.PBL_KIND_RANGEKEYDEL, N.PBL_KIND_RANGEKEYUNSET, N.PBL_KIND_RANGEKEYSET
MASKED = N.PBL_RANGEDEL_ALL


def suffix_compare(comparer: int, a: bytes, b: bytes) -> int:
    """Comparer.CompareRangeSuffixes (pbl_range_suffix_compare)."""
    return int(N.lib().pbl_range_suffix_compare(comparer, bytes(a), len(a), bytes(b), len(b)))


def _host_in(h: dict, keep: list):
    """(pbl_decode_out, pbl_keyspan_extra) over a `Decoded.to_host()` dict, capacities = what it holds."""
    d = host_struct(h, keep)
    d.kv_cap, d.key_cap, d.val_cap = int(h["n_kv"]), int(h["key_bytes_total"]), int(h["val_bytes_total"])
    x = N.KeyspanExtraC()
    for k in EXTRA_KEYS:
        a = np.ascontiguousarray(h[k] if h[k].size else np.zeros(1, h[k].dtype))
        keep.append(a)
        setattr(x, k, a.ctypes.data)
    x.suffix_cap, x.value_cap = int(h["blk_suffix_base"][-1]), int(h["blk_value_base"][-1])
    return d, x


def _runs_struct(hosts: Sequence[dict], comparer: int, snapshot: int, keep: list) -> N.RangekeyRunsC:
    pairs = [_host_in(h, keep) for h in hosts]
    n = max(len(pairs), 1)
    arr = (N.DecodeOutC * n)(*[p[0] for p in pairs])
    ext = (N.KeyspanExtraC * n)(*[p[1] for p in pairs])
    cnt = (ctypes.c_uint64 * n)(*[int(h["n_kv"]) for h in hosts])
    keep += [arr, ext, cnt]
    return N.RangekeyRunsC(ctypes.cast(arr, ctypes.POINTER(N.DecodeOutC)), ctypes.cast(ext, ctypes.POINTER(N.KeyspanExtraC)),
                           ctypes.cast(cnt, ctypes.POINTER(ctypes.c_uint64)), len(pairs), comparer, snapshot)


def _host_out(call, nb: int, cap: Optional[Capacity], extra_cap, name: str) -> dict:
    """Runs a host form that writes a decoded batch with extras: sizes first,
    then exactly, unless capacities are offered (`cap`, `extra_cap` = (suffix,
    value) bytes).  A dict in `Decoded.to_host()`'s layout."""

    def run(cap, ecap):
        r = {k: np.zeros(nb + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
        r["blk_status"] = np.zeros(max(nb, 1), np.uint32)
        xa = {"blk_suffix_base": np.zeros(nb + 1, np.uint64), "blk_value_base": np.zeros(nb + 1, np.uint64)}
        arrays = {}
        if cap is not None:
            arrays = {"trailer": np.zeros(max(cap.kv, 1), np.uint64), "kv_flags": np.zeros(max(cap.kv, 1), np.uint8),
                      "entry_off": np.zeros(max(cap.kv, 1), np.uint32),
                      "key_off": np.zeros(cap.kv + nb + 1, np.uint32), "val_off": np.zeros(cap.kv + nb + 1, np.uint32),
                      "key_bytes": np.zeros(max(cap.key, 1), np.uint8), "val_bytes": np.zeros(max(cap.val, 1), np.uint8)}
            xa.update(span=np.zeros(max(cap.kv, 1), np.uint32), suffix_off=np.zeros(cap.kv + nb + 1, np.uint32),
                      value_off=np.zeros(cap.kv + nb + 1, np.uint32), suffix_bytes=np.zeros(max(ecap[0], 1), np.uint8),
                      value_bytes=np.zeros(max(ecap[1], 1), np.uint8))
        tot = N.TotalsC()
        o, x = N.DecodeOutC(), N.KeyspanExtraC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        for k, a in xa.items():
            setattr(x, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        if cap is not None:
            o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
            x.suffix_cap, x.value_cap = int(ecap[0]), int(ecap[1])
        rc = call(o, x)
        if rc != N.PBL_OK:
            raise DecodeError(f"{name} failed: {N.STATUS_NAMES.get(rc, rc)}")
        return r, arrays, xa, tot

    if cap is None or extra_cap is None:
        _, _, xa, tot = run(None, None)
        cap = cap or Capacity(int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes), 0)
        extra_cap = extra_cap if extra_cap is not None else (int(xa["blk_suffix_base"][nb]), int(xa["blk_value_base"][nb]))
    r, arrays, xa, tot = run(cap, extra_cap)
    over = bool(tot.status_mask & (1 << N.PBL_OVERFLOW))
    n, kb, vb = (0, 0, 0) if over else (int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes))
    no = 0 if over else n + nb
    sb, xb = (0, 0) if over else (int(xa["blk_suffix_base"][nb]), int(xa["blk_value_base"][nb]))
    res = {"trailer": arrays["trailer"][:n], "kv_flags": arrays["kv_flags"][:n], "entry_off": arrays["entry_off"][:n],
           "key_off": arrays["key_off"][:no], "val_off": arrays["val_off"][:no], "key_bytes": arrays["key_bytes"][:kb],
           "val_bytes": arrays["val_bytes"][:vb], "restarts": None, **r}
    res["blk_status"] = r["blk_status"][:nb]
    res.update(n_kv=int(tot.n_kv), key_bytes_total=int(tot.key_bytes), val_bytes_total=int(tot.val_bytes), n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    res.update(span=xa["span"][:n], suffix_off=xa["suffix_off"][:no], value_off=xa["value_off"][:no],
               suffix_bytes=xa["suffix_bytes"][:sb], value_bytes=xa["value_bytes"][:xb],
               blk_suffix_base=xa["blk_suffix_base"], blk_value_base=xa["blk_value_base"])
    return res


def build_set_host(hosts: Sequence[dict], comparer: int, snapshot: int = SEQNUM_MAX, cap: Optional[Capacity] = None,
                   extra_cap: Optional[Sequence[int]] = None) -> dict:
    """The coalesced, defragmented set of the runs (`Decoded.to_host()` dicts) at
    `snapshot` (pbl_rangekey_set_host), as a dict in `Decoded.to_host()`'s layout.
    The set's status is in `blk_status[0]` and `status_mask`; a set with a status
    is empty.  `cap` / `extra_cap`: capacities to offer instead of the exact ones."""
    hosts = list(hosts)
    keep: list = []
    rs = _runs_struct(hosts, comparer, snapshot, keep)
    lib = N.lib()
    res = _host_out(lambda o, x: lib.pbl_rangekey_set_host(ctypes.byref(rs), ctypes.byref(o), ctypes.byref(x)), 1, cap,
                    extra_cap, "pbl_rangekey_set_host")
    del keep
    return res


def _ranges(lowers, uppers, comparer: int, keep: list) -> N.ScanQueriesC:
    n = len(lowers)
    if len(uppers) != n:
        raise ValueError("one upper (or None) per lower")
    lo = [bytes(k) if k is not None else b"" for k in lowers]
    up = [bytes(k) if k is not None else b"" for k in uppers]
    lb = np.frombuffer(b"".join(lo) + b"\0", np.uint8).copy()
    ub = np.frombuffer(b"".join(up) + b"\0", np.uint8).copy()
    lo_off = np.cumsum([0] + [len(k) for k in lo]).astype(np.uint64)
    up_off = np.cumsum([0] + [len(k) for k in up]).astype(np.uint64)
    fl = np.array([N.PBL_SCAN_NO_UPPER if k is None else 0 for k in uppers] or [0], np.uint8)
    keep += [lb, ub, lo_off, up_off, fl]
    return N.ScanQueriesC(lb.ctypes.data, lo_off.ctypes.data, ub.ctypes.data, up_off.ctypes.data, fl.ctypes.data, None, n,
                          comparer, 0, 0)


def clip_host(set_host: dict, lowers: Sequence[Optional[bytes]], uppers: Sequence[Optional[bytes]], comparer: int,
              cap: Optional[Capacity] = None, extra_cap: Optional[Sequence[int]] = None) -> dict:
    """One block per range [lower, upper) (None = unbounded): the set's spans that
    intersect it, truncated to it (pbl_rangekey_clip_host), in the set's form."""
    keep: list = []
    d, x = _host_in(set_host, keep)
    q = _ranges(list(lowers), list(uppers), comparer, keep)
    lib = N.lib()
    res = _host_out(lambda o, ox: lib.pbl_rangekey_clip_host(ctypes.byref(d), ctypes.byref(x), ctypes.byref(q),
                                                             ctypes.byref(o), ctypes.byref(ox)),
                    len(lowers), cap, extra_cap, "pbl_rangekey_clip_host")
    del keep
    return res


def to_device(host: dict, device) -> Decoded:
    """A set (or a clipped batch, or a run) built on the host as a `Decoded` on
    the device: what `mask()` reads."""
    nb = len(host["blk_status"])
    over = bool(host["status_mask"] & (1 << N.PBL_OVERFLOW))
    n = 0 if over else int(host["n_kv"])
    cap = Capacity(n, 0 if over else int(host["key_bytes_total"]), 0 if over else int(host["val_bytes_total"]), 0)
    sb, vb = (0, 0) if over else (int(host["blk_suffix_base"][nb]), int(host["blk_value_base"][nb]))
    dev = torch.device(device)
    out = DecodedBatch.allocate(nb, cap, dev, entry_off=True, restarts=False)
    ex = Extras.allocate(nb, n, sb, vb, dev)

    def put(t: torch.Tensor, a, dt):
        a = np.ascontiguousarray(a)
        if a.size:
            t[: a.size].copy_(torch.from_numpy(a.view(dt).copy()))

    for k, dt in (("trailer", np.int64), ("kv_flags", np.uint8), ("entry_off", np.int32), ("key_off", np.int32),
                  ("val_off", np.int32), ("key_bytes", np.uint8), ("val_bytes", np.uint8), ("blk_kv_base", np.int64),
                  ("blk_key_base", np.int64), ("blk_val_base", np.int64), ("blk_rst_base", np.int64),
                  ("blk_status", np.int32)):
        if host.get(k) is not None:
            put(getattr(out, k), host[k], dt)
    for k, dt in (("span", np.int32), ("suffix_off", np.int32), ("value_off", np.int32), ("suffix_bytes", np.uint8),
                  ("value_bytes", np.uint8), ("blk_suffix_base", np.int64), ("blk_value_base", np.int64)):
        put(getattr(ex, k), host[k], dt)
    tot = N.TotalsC(int(host["n_kv"]), int(host["key_bytes_total"]), int(host["val_bytes_total"]), 0,
                    int(host["status_mask"]), int(host["n_bad_blocks"]), 0, 0)
    out.totals.copy_(torch.from_numpy(np.frombuffer(bytes(tot), np.uint8).copy()))
    out._host_totals = tot
    return Decoded(out, ex)


def mask(set_: Decoded, batch: DecodedBatch, comparer: int, suffix: bytes, cover: Optional[torch.Tensor] = None,
         stream=None) -> torch.Tensor:
    """int64 [n_kv]: `cover` (zeros when None; a `rangedel.cover()` result is
    updated in place) with PBL_RANGEDEL_ALL stored for every KV of `batch` that
    the set masks at the threshold `suffix` (pbl_rangekey_mask).  A set with a
    status, or an empty one, masks nothing."""
    dev = batch.trailer.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    n_kv = _n_kv(batch)
    suffix = bytes(suffix)
    with torch.cuda.stream(st):
        if cover is None:
            cover = torch.zeros(max(n_kv, 1), dtype=torch.int64, device=dev)[:n_kv]
        t = torch.zeros(len(suffix) + 16, dtype=torch.uint8, device=dev)
        if suffix:
            t[: len(suffix)].copy_(torch.from_numpy(np.frombuffer(suffix, np.uint8).copy()), non_blocking=False)
    if cover.dtype != torch.int64 or cover.device != dev or cover.numel() < n_kv or not cover.is_contiguous():
        raise ValueError("cover: a contiguous int64 tensor of n_kv entries on the batch's device")
    sc, xc, bc = set_.batch.c_struct(), set_.extras.c_struct(), batch.c_struct()
    rc = N.lib().pbl_rangekey_mask(ctypes.byref(sc), ctypes.byref(xc), ctypes.byref(bc), batch.n_blocks, n_kv, comparer,
                                   ctypes.c_void_p(t.data_ptr()), len(suffix), ctypes.c_void_p(cover.data_ptr()),
                                   ctypes.c_void_p(st.cuda_stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangekey_mask failed: {N.STATUS_NAMES.get(rc, rc)}")
    return cover[:n_kv]


def _cover_in(batch: dict, cover) -> np.ndarray:
    n = int(batch["n_kv"])
    out = np.zeros(max(n, 1), np.uint64)
    if cover is not None:
        out[:n] = np.asarray(cover, np.uint64)[:n]
    return out


def mask_set_host(set_host: dict, batch: dict, comparer: int, suffix: bytes, cover=None) -> np.ndarray:
    """uint64 [n_kv]: the same lookup over host arrays (pbl_rangekey_mask_set_host)."""
    keep: list = []
    d, x = _host_in(set_host, keep)
    b = host_struct(batch, keep)
    out = _cover_in(batch, cover)
    suffix = bytes(suffix)
    rc = N.lib().pbl_rangekey_mask_set_host(ctypes.byref(d), ctypes.byref(x), ctypes.byref(b), len(batch["blk_status"]),
                                            comparer, suffix, len(suffix), out.ctypes.data)
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangekey_mask_set_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    del keep
    return out[: int(batch["n_kv"])]


def mask_host(hosts: Sequence[dict], batch: dict, comparer: int, suffix: bytes, snapshot: int = SEQNUM_MAX, cover=None):
    """(uint64 [n_kv], status): every KV of the host batch against every fragment
    of the RUNS (pbl_rangekey_mask_host), and the status their set has (nothing
    is masked with a status)."""
    hosts = list(hosts)
    keep: list = []
    rs = _runs_struct(hosts, comparer, snapshot, keep)
    b = host_struct(batch, keep)
    out = _cover_in(batch, cover)
    st = ctypes.c_uint32(0)
    suffix = bytes(suffix)
    rc = N.lib().pbl_rangekey_mask_host(ctypes.byref(rs), ctypes.byref(b), len(batch["blk_status"]), suffix, len(suffix),
                                        out.ctypes.data, ctypes.byref(st))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_rangekey_mask_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    del keep
    return out[: int(batch["n_kv"])], int(st.value)
