"""Table bloom filters: batched probes on the device.

Get and SeekPrefixGE ask a table's filter before they touch an index or data
block (sstable/reader_iter_single_lvl.go:1037-1134).  `probe()` asks that
question for a batch of keys against one or many filter blocks in one
stream-ordered launch (pbl_filter_probe, pebble_amd/csrc/filter.hip);
`probe_host()` is the same over host memory (pbl_filter_probe_host), the
reference the device path is tested against; `build_host()` writes a filter
block (pbl_bloom_build_host) and exists to make inputs.  `get()` is a point
lookup over many tables that decodes only the tables a key may be in.  Only the
bloom family ("rocksdb.BuiltinBloomFilter") is read.  torch is plumbing here:
device memory and streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .batch import DecodeError, _stream_handle
from .seek import Keys, pack_keys

FILTER_NAME = b"fullfilter.rocksdb.BuiltinBloomFilter"  # "fullfilter." + bloom.Family (layout.go:1119)


@dataclass
class FilterResult:
    may: torch.Tensor     # uint8 [n] (which given) or [n_filters, n]: PBL_FILTER_* bits
    hash: torch.Tensor    # int32 [n] (the u32 hash of every key's Split-prefix)
    status: torch.Tensor  # int32 [n_filters]: PBL_OK / PBL_CORRUPT_FILTER


class GetResult(torch.Tensor):
    """int64 [n_tables, n] with what the filter saved."""
    n_searched_tables: int
    n_candidate_pairs: int


def pack_filters(filters: Sequence, device) -> tuple:
    """Filters (bytes or uint8 device tensors) in one device buffer: (bytes
    padded by 16, int64 offsets [F + 1])."""
    lens = [int(f.numel()) if isinstance(f, torch.Tensor) else len(f) for f in filters]
    off = np.zeros(len(filters) + 1, np.int64)
    off[1:] = np.cumsum(lens, dtype=np.int64)
    if all(not isinstance(f, torch.Tensor) for f in filters):
        buf = np.zeros(int(off[-1]) + 16, np.uint8)
        buf[: int(off[-1])] = np.frombuffer(b"".join(bytes(f) for f in filters), np.uint8)
        return torch.from_numpy(buf).to(device), torch.from_numpy(off).to(device)
    parts = [f.to(device=device, dtype=torch.uint8).reshape(-1) if isinstance(f, torch.Tensor)
             else torch.from_numpy(np.frombuffer(bytes(f), np.uint8).copy()).to(device) for f in filters]
    parts.append(torch.zeros(16, dtype=torch.uint8, device=device))
    return torch.cat(parts), torch.from_numpy(off).to(device)


def _which_array(which, n: int) -> np.ndarray:
    w = np.ascontiguousarray(which, dtype=np.uint32)
    if w.size != n:
        raise ValueError("one filter id per key")
    return w


def probe(filters: Sequence, keys: Keys, comparer: int, which=None, stream=None, device="cuda") -> FilterResult:
    """MayContain of every key's Split-prefix.  `which` (a sequence or an int32
    device tensor, one filter id per key) names the filter of each key; without
    it every key is asked of every filter, and `may` is [n_filters, n]."""
    if isinstance(keys, tuple):
        kb, ko = keys
        dev = kb.device
    else:
        dev = next((f.device for f in filters if isinstance(f, torch.Tensor)), torch.device(device))
        hb, ho = pack_keys(list(keys))
        kb = torch.from_numpy(hb).to(dev)
        ko = torch.from_numpy(ho.view(np.int64)).to(dev)
    n = int(ko.numel()) - 1
    nf = len(filters)
    fb, fo = pack_filters(filters, dev)
    w = None
    if which is not None:
        w = which if isinstance(which, torch.Tensor) else \
            torch.from_numpy(_which_array(which, n).view(np.int32)).to(dev)
        if int(w.numel()) != n:
            raise ValueError("one filter id per key")
    rows = 1 if w is not None else nf
    may = torch.empty(max(rows * n, 1), dtype=torch.uint8, device=dev)
    hs = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(max(nf, 1), dtype=torch.int32, device=dev)
    s = N.FilterSetC(fb.data_ptr(), fo.data_ptr(), nf)
    q = N.FilterQueriesC(kb.data_ptr(), ko.data_ptr(), w.data_ptr() if w is not None else None, n, comparer)
    o = N.FilterOutC(may.data_ptr(), hs.data_ptr(), st.data_ptr())
    rc = N.lib().pbl_filter_probe(ctypes.byref(s), ctypes.byref(q), ctypes.byref(o), _stream_handle(stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_filter_probe failed: {N.STATUS_NAMES.get(rc, rc)}")
    may = may[: rows * n]
    return FilterResult(may if w is not None else may.reshape(nf, n), hs[:n], st[:nf])


def probe_host(filters: Sequence[bytes], keys: Sequence[bytes], comparer: int, which=None):
    """The same over host memory (pbl_filter_probe_host): (may uint8 [n] or
    [n_filters, n], hash uint32 [n], status int32 [n_filters]) as numpy."""
    kb, ko = pack_keys(list(keys))
    kb = np.ascontiguousarray(kb[: max(int(ko[-1]), 1)])  # the host form reads nothing past a key
    n, nf = len(ko) - 1, len(filters)
    off = np.zeros(nf + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in filters], dtype=np.uint64)
    fb = np.frombuffer(b"".join(bytes(f) for f in filters) or b"\0", np.uint8).copy()
    w = _which_array(which, n) if which is not None else None
    rows = 1 if w is not None else nf
    may = np.zeros(max(rows * n, 1), np.uint8)
    hs = np.zeros(max(n, 1), np.uint32)
    st = np.zeros(max(nf, 1), np.int32)
    s = N.FilterSetC(fb.ctypes.data, off.ctypes.data, nf)
    q = N.FilterQueriesC(kb.ctypes.data, ko.ctypes.data, w.ctypes.data if w is not None else None, n, comparer)
    o = N.FilterOutC(may.ctypes.data, hs.ctypes.data, st.ctypes.data)
    rc = N.lib().pbl_filter_probe_host(ctypes.byref(s), ctypes.byref(q), ctypes.byref(o))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_filter_probe_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    may = may[: rows * n]
    return (may if w is not None else may.reshape(nf, n)), hs[:n], st[:nf]


def build_host(keys: Sequence[bytes], comparer: int, bits_per_key: int) -> bytes:
    """The filter block a table writer with bloom.FilterPolicy(bits_per_key)
    writes for `keys` in this order (b"" for no keys)."""
    lib = N.lib()
    kb, ko = pack_keys(list(keys))
    n = len(ko) - 1
    cap = int(lib.pbl_bloom_build_bound(n, bits_per_key))
    out = np.zeros(max(cap, 1), np.uint8)
    ln = ctypes.c_uint64(0)
    rc = lib.pbl_bloom_build_host(kb.ctypes.data, ko.ctypes.data, n, comparer, bits_per_key, out.ctypes.data, cap,
                                  ctypes.byref(ln))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_bloom_build_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    return out[: ln.value].tobytes()


def get(tables: Sequence, keys: Keys, use_filter: bool = True) -> GetResult:
    """Row t is `tables[t].get(keys)`: int64 [len(tables), n].  With the filter,
    one all-pairs probe over the tables' filter blocks runs first; a table in
    which no key may be present is not decoded, the others are searched, and
    the pairs the filter excludes are -1.  A table without a bloom filter
    excludes nothing.  All tables share one comparer and one device.  The
    result carries `n_searched_tables` and `n_candidate_pairs`."""
    nt = len(tables)
    if nt == 0:
        raise ValueError("no tables")
    dev = tables[0].device
    if isinstance(keys, tuple):
        kb, ko = keys
    else:
        hb, ho = pack_keys(list(keys))
        kb = torch.from_numpy(hb).to(dev)
        ko = torch.from_numpy(ho.view(np.int64)).to(dev)
    n = int(ko.numel()) - 1
    out = torch.full((nt, n), -1, dtype=torch.int64, device=dev)
    may = torch.ones((nt, n), dtype=torch.bool, device=dev)
    if use_filter:
        comparer = tables[0].comparer()
        if any(t.comparer() != comparer for t in tables[1:]):
            raise ValueError("the tables have different comparers")
        flt = [t.filter() for t in tables]
        have = [i for i, f in enumerate(flt) if f is not None]
        if have and n:
            r = probe([flt[i] for i in have], (kb, ko), comparer)
            may[torch.tensor(have, device=dev)] = (r.may & N.PBL_FILTER_MAY) != 0
    searched = may.any(dim=1).cpu().tolist() if n else [False] * nt
    for t in range(nt):
        if searched[t]:
            g = tables[t].get((kb, ko))
            out[t] = torch.where(may[t], g, out[t])
    res = out.as_subclass(GetResult)
    res.n_searched_tables = int(sum(searched))
    res.n_candidate_pairs = int(may.sum().item()) if n else 0
    return res
