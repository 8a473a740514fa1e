"""Batched SeekGE / SeekLT over a decoded batch (device side).

`seek()` positions many keys in one stream-ordered launch over a
`DecodedBatch` in HBM (pbl_seek_batch, pebble_amd/csrc/seek.hip): per-block mode
is blockiter.Data.SeekGE / SeekLT in a named block, table mode is
singleLevelIterator.SeekGE / SeekLT over the whole batch (include/pebble_amd.h
states both).  `prepare()` builds table mode's fence table once
(pbl_seek_prepare); `seek_host()` runs the same search over host arrays
(pbl_seek_batch_host), the reference the device path is tested against.
torch is plumbing here: device memory and streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N
from .batch import DecodedBatch, DecodeError, _stream_handle

OPS = {"ge": N.PBL_SEEK_GE, "lt": N.PBL_SEEK_LT}
Keys = Union[Sequence[bytes], Tuple[torch.Tensor, torch.Tensor]]


@dataclass
class SeekIndex:
    """The fence table of one decoded batch under one comparer (read-only)."""
    workspace: torch.Tensor  # uint8, device
    comparer: int
    n_blocks: int


@dataclass
class SeekResult:
    kv: torch.Tensor     # int64 [n]: global KV index, or -1 (PBL_SEEK_NONE as int64)
    block: torch.Tensor  # int32 [n]: block of the landing KV
    flags: torch.Tensor  # uint8 [n]: PBL_SEEK_* bits


def pack_keys(keys: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """(key bytes padded by 16, uint64 offsets [n + 1]) of a list of keys."""
    off = np.zeros(len(keys) + 1, np.uint64)
    if len(keys):
        off[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    buf = np.zeros(int(off[-1]) + 16, np.uint8)
    buf[: int(off[-1])] = np.frombuffer(b"".join(keys), np.uint8)
    return buf, off


def prepare(decoded: DecodedBatch, comparer: int, stream=None) -> SeekIndex:
    lib = N.lib()
    nb = decoded.n_blocks
    ws = torch.empty(int(lib.pbl_seek_workspace_bytes(nb)), dtype=torch.uint8, device=decoded.trailer.device)
    o = decoded.c_struct()
    rc = lib.pbl_seek_prepare(ctypes.byref(o), nb, comparer, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                              _stream_handle(stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_seek_prepare failed: {N.STATUS_NAMES.get(rc, rc)}")
    return SeekIndex(ws, comparer, nb)


def seek(decoded: DecodedBatch, keys: Keys, *, op: str = "ge", comparer: int,
         blocks=None, hide_obsolete_points: bool = False, index: Optional[SeekIndex] = None,
         stream=None, filter: Optional[torch.Tensor] = None) -> SeekResult:
    """Seek every key.  `keys`: a list of bytes, or (uint8 tensor readable 16 B
    past the last key, int64 offsets [n + 1]) already on the device.  `blocks`
    (a sequence or an int32 device tensor, one block id per key) selects
    per-block mode; without it the seek is over the whole batch, with `index`
    or an index built here.  `filter` (a table's bloom filter block, a uint8
    device tensor; table mode and "ge" only) makes it SeekPrefixGE: a key whose
    Split-prefix the filter excludes is answered -1 with PBL_SEEK_FILTERED and
    not searched (pbl_seek_prefix_batch)."""
    dev = decoded.trailer.device
    if isinstance(keys, tuple):
        kb, ko = keys
    else:
        hb, ho = pack_keys(list(keys))
        kb = torch.from_numpy(hb).to(dev)
        ko = torch.from_numpy(ho.view(np.int64)).to(dev)
    n = int(ko.numel()) - 1
    blk = None
    if blocks is not None:
        blk = blocks if isinstance(blocks, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.uint32).view(np.int32)).to(dev)
        if int(blk.numel()) != n:
            raise ValueError("one block id per key")
    elif index is None:
        index = prepare(decoded, comparer, stream)
    if index is not None and blk is None and (index.comparer != comparer or index.n_blocks != decoded.n_blocks):
        raise ValueError("the SeekIndex was prepared for another comparer or batch")
    kv = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    ob = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    fl = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    q = N.SeekQueriesC(kb.data_ptr(), ko.data_ptr(), blk.data_ptr() if blk is not None else None, n, comparer,
                       OPS[op], 1 if hide_obsolete_points else 0)
    out = N.SeekOutC(kv.data_ptr(), ob.data_ptr(), fl.data_ptr())
    o = decoded.c_struct()
    ws = index.workspace if (index is not None and blk is None) else None
    wp, wn = (ctypes.c_void_p(ws.data_ptr()), ws.numel()) if ws is not None else (None, 0)
    if filter is not None:
        rc = N.lib().pbl_seek_prefix_batch(ctypes.byref(o), decoded.n_blocks, ctypes.byref(q),
                                           ctypes.c_void_p(filter.data_ptr()), int(filter.numel()),
                                           ctypes.byref(out), wp, wn, _stream_handle(stream))
    else:
        rc = N.lib().pbl_seek_batch(ctypes.byref(o), decoded.n_blocks, ctypes.byref(q), ctypes.byref(out), wp, wn,
                                    _stream_handle(stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_seek_batch failed: {N.STATUS_NAMES.get(rc, rc)}")
    return SeekResult(kv[:n], ob[:n], fl[:n])


def seek_host(host: dict, keys: Sequence[bytes], *, op: str = "ge", comparer: int, blocks=None,
              hide_obsolete_points: bool = False, filter: Optional[bytes] = None):
    """The same seek over host arrays (`DecodedBatch.to_host()` or the
    oracle's dict) through pbl_seek_batch_host: (kv uint64 with PBL_SEEK_NONE,
    block uint32, flags uint8) as numpy."""
    nb = len(host["blk_status"])
    keep = {}
    o = N.DecodeOutC()
    for k in ("kv_flags", "key_off", "key_bytes", "blk_kv_base", "blk_key_base", "blk_status"):
        a = host[k]
        a = np.ascontiguousarray(a if a is not None and a.size else np.zeros(1, a.dtype if a is not None
                                                                             else np.uint8))
        keep[k] = a
        setattr(o, k, a.ctypes.data)
    kb, ko = pack_keys(list(keys))
    n = len(ko) - 1
    blk = np.ascontiguousarray(blocks, dtype=np.uint32) if blocks is not None else None
    kv = np.empty(max(n, 1), np.uint64)
    ob = np.empty(max(n, 1), np.uint32)
    fl = np.empty(max(n, 1), np.uint8)
    q = N.SeekQueriesC(kb.ctypes.data, ko.ctypes.data, blk.ctypes.data if blk is not None else None, n, comparer,
                       OPS[op], 1 if hide_obsolete_points else 0)
    out = N.SeekOutC(kv.ctypes.data, ob.ctypes.data, fl.ctypes.data)
    if filter is not None:  # pbl_seek_prefix_batch_host: SeekPrefixGE behind the table's bloom filter
        fb = np.frombuffer(bytes(filter) or b"\0", np.uint8)
        rc = N.lib().pbl_seek_prefix_batch_host(ctypes.byref(o), nb, ctypes.byref(q), fb.ctypes.data, len(filter),
                                                ctypes.byref(out))
    else:
        rc = N.lib().pbl_seek_batch_host(ctypes.byref(o), nb, ctypes.byref(q), ctypes.byref(out))
    if rc != N.PBL_OK:
        raise DecodeError(f"pbl_seek_batch_host failed: {N.STATUS_NAMES.get(rc, rc)}")
    return kv[:n], ob[:n], fl[:n]
