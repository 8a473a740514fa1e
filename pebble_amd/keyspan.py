"""Columnar keyspan blocks on the device.

A columnar table (Pebblev5 and later) keeps its range deletions, and its range
keys, in colblk keyspan blocks (sstable/colblk/keyspan.go).  `decode()` turns a
batch of them into *runs* as `pebble_amd.rangedel` defines them (key = start,
trailer, value = end, one KV per keyspan.Key, one result block per input block;
pbl_keyspan_size + pbl_keyspan_decode, pebble_amd/csrc/keyspan.hip), which
`rangedel.build_set`, `to_host()`, `DataIter` and the per-block seeks read
unchanged.  `extras=True` also returns, per KV, the span's boundary index and
the keyspan.Key's suffix and value, which range keys need.  `size()` is the
size-only call, `decode_host()` the host form (the reference's sequential
walk, pbl_keyspan_decode_host).  `Writer` is an encoder for tests and tools, a
Python restatement of KeyspanBlockWriter.AddSpan / Finish (keyspan.go:91-190);
only the decoder is a hot path.  torch is plumbing here: device memory and
streams."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .batch import BlockBatch, Capacity, DecodedBatch, DecodeError

EXTRA_KEYS = ("span", "suffix_off", "value_off", "suffix_bytes", "value_bytes", "blk_suffix_base", "blk_value_base")


@dataclass
class Extras:
    """Per KV of a decoded keyspan batch: the start boundary index of its span,
    and the keyspan.Key's Suffix and Value, laid out as keys are (offsets relative
    to the block's base, n_kv + n_blocks of them)."""
    span: torch.Tensor
    suffix_off: torch.Tensor
    value_off: torch.Tensor
    suffix_bytes: torch.Tensor
    value_bytes: torch.Tensor
    blk_suffix_base: torch.Tensor
    blk_value_base: torch.Tensor
    suffix_cap: int
    value_cap: int

    @classmethod
    def allocate(cls, n_blocks: int, kv: int, suffix: int, value: int, device) -> "Extras":
        u = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=device)  # noqa: E731
        return cls(u(kv, torch.int32), u(kv + n_blocks, torch.int32), u(kv + n_blocks, torch.int32),
                   u(suffix + 16, torch.uint8), u(value + 16, torch.uint8), u(n_blocks + 1, torch.int64),
                   u(n_blocks + 1, torch.int64), int(suffix), int(value))

    def c_struct(self) -> N.KeyspanExtraC:
        return N.KeyspanExtraC(self.span.data_ptr(), self.suffix_off.data_ptr(), self.value_off.data_ptr(),
                               self.suffix_bytes.data_ptr(), self.value_bytes.data_ptr(),
                               self.blk_suffix_base.data_ptr(), self.blk_value_base.data_ptr(), self.suffix_cap,
                               self.value_cap)

    def to_host(self, n_kv: int, n_blocks: int) -> dict:
        base_s = self.blk_suffix_base[: n_blocks + 1].cpu().numpy().view(np.uint64)
        base_v = self.blk_value_base[: n_blocks + 1].cpu().numpy().view(np.uint64)
        g = lambda x, k, dt: x[:k].cpu().numpy().view(dt) if k else np.zeros(0, dt)  # noqa: E731
        return {"span": g(self.span, n_kv, np.uint32), "suffix_off": g(self.suffix_off, n_kv + n_blocks, np.uint32),
                "value_off": g(self.value_off, n_kv + n_blocks, np.uint32),
                "suffix_bytes": g(self.suffix_bytes, int(base_s[-1]), np.uint8),
                "value_bytes": g(self.value_bytes, int(base_v[-1]), np.uint8),
                "blk_suffix_base": base_s, "blk_value_base": base_v}


class Decoded(NamedTuple):
    """What `decode(..., extras=True)` returns."""
    batch: DecodedBatch
    extras: Extras

    def to_host(self) -> dict:
        r = self.batch.to_host()
        over = bool(r["status_mask"] & (1 << N.PBL_OVERFLOW))
        r.update(self.extras.to_host(0 if over else r["n_kv"], self.batch.n_blocks))
        return r


def total_boundaries(batch: BlockBatch) -> int:
    """The sum over the blocks of min(B, block length), B being each block's
    first four bytes: what the workspace is sized by (one small copy to the host)."""
    nb = batch.n_blocks
    if nb == 0:
        return 0
    lens = batch.block_len.to(torch.int64) & 0xFFFFFFFF
    at = batch.block_off.view(-1, 1) + torch.arange(4, device=batch.device, dtype=torch.int64).view(1, -1)
    at = torch.minimum(at, torch.tensor(batch.blocks.numel() - 1, device=batch.device))
    raw = batch.blocks[at].to(torch.int64)
    b = raw[:, 0] | raw[:, 1] << 8 | raw[:, 2] << 16 | raw[:, 3] << 24
    b = torch.where(lens >= 4, b, torch.zeros_like(b))
    return int(torch.minimum(b, lens).sum().item())


def _run(batch: BlockBatch, out: DecodedBatch, ex: Optional[Extras], ws: torch.Tensor, tb: int, st, size_only: bool):
    b, o = batch.c_struct(), out.c_struct()
    x = ex.c_struct() if ex is not None else None
    fn = N.lib().pbl_keyspan_size if size_only else N.lib().pbl_keyspan_decode
    rc = fn(ctypes.byref(b), tb, ctypes.byref(o), ctypes.byref(x) if x is not None else None,
            ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(st.cuda_stream))
    if rc != N.PBL_OK:
        raise DecodeError(f"{'pbl_keyspan_size' if size_only else 'pbl_keyspan_decode'} failed: "
                          f"{N.STATUS_NAMES.get(rc, rc)}")


def _workspace(batch: BlockBatch, tb: int, st) -> torch.Tensor:
    with torch.cuda.stream(st):
        return torch.empty(int(N.lib().pbl_keyspan_workspace_bytes(batch.n_blocks, tb)), dtype=torch.uint8,
                           device=batch.device)


def _size(batch: BlockBatch, extras: bool, st, tb: int, ws: torch.Tensor):
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(batch.n_blocks, Capacity(0, 0, 0, 0), batch.device, entry_off=False,
                                    restarts=False)
        ex = Extras.allocate(batch.n_blocks, 0, 0, 0, batch.device) if extras else None
    _run(batch, out, ex, ws, tb, st, True)
    st.synchronize()
    t = out.read_totals()
    nb = batch.n_blocks
    sb = int(ex.blk_suffix_base[nb].item()) if extras else 0
    vb = int(ex.blk_value_base[nb].item()) if extras else 0
    return out, t, sb, vb


def size(batch: BlockBatch, extras: bool = False, stream=None) -> dict:
    """The size-only call: the totals a decode of `batch` has (n_kv, key_bytes,
    val_bytes, status_mask, n_bad_blocks; with `extras` also suffix_bytes and
    value_bytes), and blk_status."""
    st = stream if stream is not None else torch.cuda.current_stream(batch.device)
    tb = total_boundaries(batch)
    out, t, sb, vb = _size(batch, extras, st, tb, _workspace(batch, tb, st))
    r = {"n_kv": int(t.n_kv), "key_bytes": int(t.key_bytes), "val_bytes": int(t.val_bytes),
         "status_mask": int(t.status_mask), "n_bad_blocks": int(t.n_bad_blocks),
         "blk_status": out.blk_status[: batch.n_blocks].cpu().numpy().view(np.uint32)}
    if extras:
        r.update(suffix_bytes=sb, value_bytes=vb)
    return r


def decode(batch: BlockBatch, extras: bool = False, stream=None, cap: Optional[Capacity] = None,
           extra_cap: Optional[Sequence[int]] = None):
    """Decode a batch of keyspan blocks into runs: a `DecodedBatch` with one block
    per input block, or with `extras` a `Decoded(batch, extras)`.  The size call
    runs first, so the result is allocated exactly; `cap` / `extra_cap` (suffix,
    value bytes) offer other capacities instead (PBL_OVERFLOW in the totals when
    one is too small).  Per-block corruption is in blk_status and the totals."""
    st = stream if stream is not None else torch.cuda.current_stream(batch.device)
    tb = total_boundaries(batch)
    ws = _workspace(batch, tb, st)
    if cap is None or (extras and extra_cap is None):
        _, t, sb, vb = _size(batch, extras, st, tb, ws)
        cap = cap or Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=0)
        extra_cap = extra_cap if extra_cap is not None else (sb, vb)
    with torch.cuda.stream(st):
        out = DecodedBatch.allocate(batch.n_blocks, cap, batch.device, entry_off=True, restarts=False)
        ex = Extras.allocate(batch.n_blocks, cap.kv, extra_cap[0], extra_cap[1], batch.device) if extras else None
    _run(batch, out, ex, ws, tb, st, False)
    out.source = batch
    st.synchronize()
    out.read_totals()
    return Decoded(out, ex) if extras else out


def decode_host(blocks: Sequence[bytes], extras: bool = False, synthetic_seq_num: int = 0,
                cap: Optional[Capacity] = None, extra_cap: Optional[Sequence[int]] = None) -> dict:
    """The host form over a list of block byte strings (pbl_keyspan_decode_host),
    as a dict in `to_host()`'s layout (with `extras`, the EXTRA_KEYS too).  Without
    `cap` it sizes first and allocates exactly."""
    blocks = [bytes(b) for b in blocks]
    nb = len(blocks)
    offs, pos = [], 0
    for bk in blocks:
        offs.append(pos)
        pos += len(bk)
    buf = np.frombuffer(b"".join(blocks) or b"\0", np.uint8).copy()
    off = np.array(offs or [0], np.uint64)
    lens = np.array([len(b) for b in blocks] or [0], np.uint32)
    bb = N.BlockBatchC(buf.ctypes.data, off.ctypes.data, lens.ctypes.data, nb, 0, 0, 0, None, synthetic_seq_num)

    def call(cap, ecap):
        r = {k: np.zeros(nb + 1, np.uint64) for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base")}
        r["blk_status"] = np.zeros(max(nb, 1), np.uint32)
        arrays = {}
        if cap is not None:
            arrays = {"trailer": np.zeros(max(cap.kv, 1), np.uint64), "kv_flags": np.zeros(max(cap.kv, 1), np.uint8),
                      "entry_off": np.zeros(max(cap.kv, 1), np.uint32),
                      "key_off": np.zeros(cap.kv + nb + 1, np.uint32), "val_off": np.zeros(cap.kv + nb + 1, np.uint32),
                      "key_bytes": np.zeros(max(cap.key, 1), np.uint8), "val_bytes": np.zeros(max(cap.val, 1), np.uint8)}
        tot = N.TotalsC()
        o = N.DecodeOutC()
        for k, a in {**r, **arrays}.items():
            setattr(o, k, a.ctypes.data)
        o.totals = ctypes.addressof(tot)
        if cap is not None:
            o.kv_cap, o.key_cap, o.val_cap = cap.kv, cap.key, cap.val
        x, xa = None, {}
        if extras:
            xa = {"blk_suffix_base": np.zeros(nb + 1, np.uint64), "blk_value_base": np.zeros(nb + 1, np.uint64)}
            if cap is not None:
                xa.update(span=np.zeros(max(cap.kv, 1), np.uint32), suffix_off=np.zeros(cap.kv + nb + 1, np.uint32),
                          value_off=np.zeros(cap.kv + nb + 1, np.uint32),
                          suffix_bytes=np.zeros(max(ecap[0], 1), np.uint8),
                          value_bytes=np.zeros(max(ecap[1], 1), np.uint8))
            x = N.KeyspanExtraC()
            for k, a in xa.items():
                setattr(x, k, a.ctypes.data)
            if cap is not None:
                x.suffix_cap, x.value_cap = int(ecap[0]), int(ecap[1])
        rc = N.lib().pbl_keyspan_decode_host(ctypes.byref(bb), ctypes.byref(o), ctypes.byref(x) if x is not None else None)
        if rc != N.PBL_OK:
            raise DecodeError(f"pbl_keyspan_decode_host failed: {N.STATUS_NAMES.get(rc, rc)}")
        return r, arrays, xa, tot

    if cap is None or (extras and extra_cap is None):
        _, _, xa, tot = call(None, None)
        cap = cap or Capacity(int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes), 0)
        if extras and extra_cap is None:
            extra_cap = (int(xa["blk_suffix_base"][nb]), int(xa["blk_value_base"][nb]))
    r, arrays, xa, tot = call(cap, extra_cap)
    over = bool(tot.status_mask & (1 << N.PBL_OVERFLOW))
    n, kb, vb = (0, 0, 0) if over else (int(tot.n_kv), int(tot.key_bytes), int(tot.val_bytes))
    no = 0 if over else n + nb
    res = {"trailer": arrays["trailer"][:n], "kv_flags": arrays["kv_flags"][:n], "entry_off": arrays["entry_off"][:n],
           "key_off": arrays["key_off"][:no], "val_off": arrays["val_off"][:no], "key_bytes": arrays["key_bytes"][:kb],
           "val_bytes": arrays["val_bytes"][:vb], "restarts": None, **r}
    res["blk_status"] = r["blk_status"][:nb]
    res.update(n_kv=int(tot.n_kv), key_bytes_total=int(tot.key_bytes), val_bytes_total=int(tot.val_bytes), n_restarts=0,
               status_mask=int(tot.status_mask), n_bad_blocks=int(tot.n_bad_blocks), n_slow_blocks=0)
    if extras:
        sb, xb = (0, 0) if over else (int(xa["blk_suffix_base"][nb]), int(xa["blk_value_base"][nb]))
        res.update(span=xa["span"][:n], suffix_off=xa["suffix_off"][:no], value_off=xa["value_off"][:no],
                   suffix_bytes=xa["suffix_bytes"][:sb], value_bytes=xa["value_bytes"][:xb],
                   blk_suffix_base=xa["blk_suffix_base"], blk_value_base=xa["blk_value_base"])
    return res


# ---- the encoder: KeyspanBlockWriter (keyspan.go:91-190) -------------------------------------------
_DT_UINT, _DT_BYTES = 2, 3
_ROW_THRESHOLD = 8  # UintEncodingRowThreshold


def _byte_width(v: int) -> int:
    n = v.bit_length()
    return 0 if n == 0 else 1 if n <= 8 else 2 if n <= 16 else 4 if n <= 32 else 8


def _uint_encoding(lo: int, hi: int, rows: int):
    """DetermineUintEncoding (uints.go:94-111): (width, delta)."""
    b = _byte_width(hi - lo)
    if b == 8:
        return 8, False
    delta = hi >= 1 << (b << 3)
    if delta and rows < _ROW_THRESHOLD:
        nb = _byte_width(hi)
        if rows * (nb - b) < 8:
            b, delta = nb, False
    return b, delta


def _put_uints(buf: bytearray, vals: Sequence[int], force=None) -> None:
    """UintBuilder.Finish (uints.go:356-430) at the end of `buf`.  `force`:
    (width, delta) instead of the smallest encoding, for tests."""
    if not vals:
        return
    lo, hi = min(vals), max(vals)
    w, delta = force if force is not None else _uint_encoding(lo, hi, len(vals))
    buf.append(w | (0x80 if delta else 0))
    base = 0
    if delta:
        base = lo
        buf += lo.to_bytes(8, "little")
    if w == 0:
        return
    while len(buf) % w:
        buf.append(0)
    for v in vals:
        buf += (v - base).to_bytes(w, "little")


def _put_rawbytes(buf: bytearray, slices: Sequence[bytes], force=None, offsets=None) -> None:
    """RawBytesBuilder.Finish (raw_bytes.go:215-223).  `offsets`: written instead
    of the slices' own, for tests of corrupt columns."""
    if not slices:
        return
    offs = [0]
    for s in slices:
        offs.append(offs[-1] + len(s))
    _put_uints(buf, offs if offsets is None else list(offsets), force)
    for s in slices:
        buf += s


class Writer:
    """KeyspanBlockWriter: `add_span(start, end, keys)` with keys
    [(trailer, suffix, value)], fragmented and in order as AddSpan requires;
    `finish()` returns the block.  `force`: per column index an (offset or
    value width, delta) to use instead of the smallest encoding, for tests."""

    def __init__(self, force: Optional[dict] = None):
        self.bounds: list = []
        self.idx: list = []
        self.trailers: list = []
        self.suffixes: list = []
        self.values: list = []
        self.force = force or {}

    def add_span(self, start: bytes, end: bytes, keys) -> None:
        if not self.bounds or self.bounds[-1] != start:  # (the caller's comparer's Equal is bytes equality here)
            self.idx.append(len(self.trailers))
            self.bounds.append(bytes(start))
        self.idx.append(len(self.trailers) + len(keys))
        self.bounds.append(bytes(end))
        for trailer, suffix, value in keys:
            self.trailers.append(int(trailer))
            self.suffixes.append(bytes(suffix))
            self.values.append(bytes(value))

    def key_count(self) -> int:
        return len(self.trailers)

    def finish(self) -> bytes:
        return encode_block(self.bounds, self.idx, self.trailers, self.suffixes, self.values, self.force)


def encode_block(bounds, idx, trailers, suffixes, values, force=None, offsets=None) -> bytes:
    """BlockEncoder over the five keyspan columns from raw column contents (so a
    test can also write blocks that AddSpan never would).  `offsets`: per
    RawBytes column index (0, 3, 4) the offsets to write instead of the slices'
    own (rows + 1 of them; the last one must stay the data's length for the
    column to pass DecodeColumn)."""
    force = force or {}
    offsets = offsets or {}
    types = (_DT_BYTES, _DT_UINT, _DT_UINT, _DT_BYTES, _DT_BYTES)
    buf = bytearray(len(bounds).to_bytes(4, "little"))
    buf += bytes([1]) + (5).to_bytes(2, "little") + len(trailers).to_bytes(4, "little")
    hdr = len(buf)
    buf += bytes(5 * 5)
    cols = ((_put_rawbytes, bounds), (_put_uints, idx), (_put_uints, trailers), (_put_rawbytes, suffixes),
            (_put_rawbytes, values))
    for c, (put, data) in enumerate(cols):
        buf[hdr + 5 * c] = types[c]
        buf[hdr + 5 * c + 1: hdr + 5 * c + 5] = len(buf).to_bytes(4, "little")
        if put is _put_rawbytes:
            put(buf, data, force.get(c), offsets.get(c))
        else:
            put(buf, data, force.get(c))
    buf.append(0)  # the trailing padding byte
    return bytes(buf)
