#!/usr/bin/env python3
"""Range deletions in the device read path: times of pbl_rangedel_set,
pbl_rangedel_cover and the view with a cover.

Input: visible_probe.py's: --blocks config-2 row blocks, every
fourth key a user key with four versions (sequence numbers 4..1) in K = 4 runs,
scanned and merged on the device as one unbounded range.  Tombstones: T
fragments spread evenly over the user keys and dealt to 4 runs, each covering
half of its stride with sequence number 3 (the two oldest versions of a covered
user key are deleted), for T = 16, 1 Ki and 64 Ki.

Per T: pbl_rangedel_set alone, pbl_rangedel_cover alone, the view through the _rd
entry points (pbl_visible_size_rd + pbl_visible_batch_rd with PBL_VISIBLE_SIZED),
each a device-event window over repeated launches after a warm-up, --repeats
windows.  The yardstick runs in the same process before and after each window:
the unchanged pbl_visible_size + pbl_visible_batch (PBL_VISIBLE_SIZED) over the
same merge result with no tombstones.  Before a time is printed the device set
is compared with a numpy statement of it (the fragments are disjoint: sorted
starts and ends, cover 3 at a start, 0 at an end), the device cover with
np.searchsorted over the boundaries, and the view with pbl_visible_batch_host_rd
over to_host(); for T up to 1 Ki the set also with pbl_rangedel_set_host (its
brute force is quadratic).

One JSON line per measurement, printed and written to <out>/rangedel_probe.jsonl.

  python scripts/rangedel_probe.py --blocks 16384 --out profiles/rangedel
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from merge_probe import encode_run, host_kvs, timed  # noqa: E402
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.merge import merge  # noqa: E402
from pebble_amd.rangedel import build_set_host  # noqa: E402
from pebble_amd.rowblk import Writer  # noqa: E402
from pebble_amd.scan import scan  # noqa: E402
from pebble_amd.visible import visible_host  # noqa: E402
from visible_probe import KINDS, D, K, Visible, gen_blocks  # noqa: E402

SEQ = 3  # the tombstones' sequence number: versions 2 and 1 are under it


class VisibleRd(Visible):
    """Visible through the _rd entry points with a cover."""

    def __init__(self, batch, cover):
        self.cover = ctypes.c_void_p(cover.data_ptr())
        super().__init__(batch)

    def size(self):
        assert self.L.pbl_visible_size_rd(ctypes.byref(self.vin), ctypes.byref(self.so), self.wp, self.ws.numel(), 0,
                                          self.cover, self.st) == 0

    def batch(self, flags):
        assert self.L.pbl_visible_batch_rd(ctypes.byref(self.vin), ctypes.byref(self.oo), self.wp, self.ws.numel(), flags,
                                           self.cover, self.st) == 0


class RangeDel:
    """The set of `runs` and the cover of `batch`, outputs allocated once."""

    def __init__(self, runs, batch):
        self.L, self.runs, self.target = N.lib(), runs, batch
        tots = [r.read_totals() for r in runs]
        self.T = sum(int(t.n_kv) for t in tots)
        self.structs = (N.DecodeOutC * len(runs))(*[r.c_struct() for r in runs])
        self.cnt = (ctypes.c_uint64 * len(runs))(*[int(t.n_kv) for t in tots])
        self.rs = N.RangedelRunsC(ctypes.cast(self.structs, ctypes.POINTER(N.DecodeOutC)),
                                  ctypes.cast(self.cnt, ctypes.POINTER(ctypes.c_uint64)), len(runs), D, N.PBL_SEQNUM_MAX)
        self.ws = torch.empty(int(self.L.pbl_rangedel_workspace_bytes(self.T)), dtype=torch.uint8, device="cuda")
        cap = Capacity(2 * self.T, sum(int(t.key_bytes) + int(t.val_bytes) for t in tots), 0, 0)
        self.set = DecodedBatch.allocate(1, cap, "cuda", entry_off=False, restarts=False)
        self.sc = self.set.c_struct()
        self.bc = batch.c_struct()
        self.n_kv = int(batch.read_totals().n_kv)
        self.cover = torch.zeros(max(self.n_kv, 1), dtype=torch.int64, device="cuda")
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def build(self):
        assert self.L.pbl_rangedel_set(ctypes.byref(self.rs), ctypes.byref(self.sc), ctypes.c_void_p(self.ws.data_ptr()),
                                       self.ws.numel(), self.st) == 0

    def lookup(self):
        assert self.L.pbl_rangedel_cover(ctypes.byref(self.sc), ctypes.byref(self.bc), self.target.n_blocks, self.n_kv, D,
                                         ctypes.c_void_p(self.cover.data_ptr()), self.st) == 0


def run_block(frags):
    w = Writer(1)
    for s, e in frags:
        w.add(s, SEQ << 8 | N.PBL_KIND_RANGEDEL, e)
    return w.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--fragments", type=int, nargs="*", default=[16, 1 << 10, 1 << 16])
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "rangedel"))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kw):
        kw["tag"] = a.tag
        kw["blocks"] = a.blocks
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("rangedel_probe.py needs a GPU: it measures nothing without one")
    buf, off, lens, n_gen = gen_blocks(a.blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    n_gen_kv = int(d.read_totals().n_kv)
    keys, _, vals = host_kvs(d.to_host())
    n_user = n_gen_kv // K
    n_kv = n_user * K
    ukeys = keys[0:n_kv:K]
    tables = []
    for r in range(K):
        trailers = [(K - r) << 8 | KINDS[u % 3][r] for u in range(n_user)]
        tables.append(decode(BlockBatch.from_blocks(encode_run(ukeys, trailers, vals[r:n_kv:K]), "cuda", N.PBL_FMT_ROW, 0)))
    merged = merge([scan(x, [None], [None], comparer=D).batch for x in tables], comparer=D).batch
    src = int(merged.read_totals().n_kv)
    emit(what="input", user_keys=n_user, source_kvs=src, device=torch.cuda.get_device_name())
    host = merged.to_host()
    hkeys = np.frombuffer(b"".join(host_kvs(host)[0]), dtype="S16")
    assert len(hkeys) == src
    yard = Visible(merged)

    def yardstick():
        return timed(yard.size)[0] + timed(yard.emit)[0]

    for T in a.fragments:
        T = min(T, n_user // 2)
        stride = n_user // T
        frags = [(ukeys[f * stride], ukeys[f * stride + max(1, stride // 2)]) for f in range(T)]
        runs = [decode(BlockBatch.from_blocks([run_block(frags[r::4])], "cuda", N.PBL_FMT_ROW, 0)) for r in range(4)]
        rd = RangeDel(runs, merged)
        rd.build()
        rd.lookup()
        torch.cuda.synchronize()
        # the set and the cover against numpy; the view against the host
        s = rd.set.to_host()
        bounds = np.frombuffer(s["key_bytes"].tobytes(), dtype="S16")
        want_b = np.array([b for fr in frags for b in fr], dtype="S16")
        set_ok = s["status_mask"] == 0 and np.array_equal(bounds, want_b) and \
            np.array_equal(s["trailer"] >> 8, np.tile(np.array([SEQ, 0], np.uint64), T))
        if T <= 1024:
            hs = build_set_host([r.to_host() for r in runs], D)
            set_ok = set_ok and all(np.array_equal(np.asarray(s[k]).astype(np.uint64), np.asarray(hs[k]).astype(np.uint64))
                                    for k in ("trailer", "key_off", "key_bytes", "blk_kv_base", "blk_key_base"))
        at = np.searchsorted(bounds, hkeys, side="right")
        want_c = np.where(at > 0, (s["trailer"] >> 8)[np.maximum(at, 1) - 1], 0).astype(np.uint64)
        cov = rd.cover[:src].cpu().numpy().view(np.uint64)
        cover_ok = np.array_equal(cov, want_c)
        v = VisibleRd(merged, rd.cover)
        v.whole()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hres = visible_host(host, comparer=D, cover=want_c)
        host_s = time.perf_counter() - t0
        view_ok = v.same_as_host(hres)
        emit(what="check", fragments=T, set_equal=bool(set_ok), cover_equal=bool(cover_ok), view_equal_to_host=view_ok,
             boundaries=int(s["n_kv"]), covered_kvs=int((want_c > 0).sum()), deleted_kvs=int((want_c > (host["trailer"] >> 8)).sum()),
             result_kvs=v.cap.kv, yardstick_result_kvs=yard.cap.kv, host_visible_rd_seconds=host_s,
             set_workspace_bytes=rd.ws.numel())
        assert set_ok and cover_ok and view_ok
        for w in range(a.repeats):
            y0 = yardstick()
            s_set, _ = timed(rd.build)
            s_cov, _ = timed(rd.lookup)
            s_size, _ = timed(v.size)
            s_emit, _ = timed(v.emit)
            y1 = yardstick()
            y = min(y0, y1)
            emit(what="rangedel", fragments=T, window=w, set_seconds=s_set, cover_seconds=s_cov, size_rd_seconds=s_size,
                 sized_batch_rd_seconds=s_emit, yardstick_seconds=y0, yardstick_again_seconds=y1, source_kvs=src,
                 cover_ns_per_kv=s_cov / src * 1e9, view_rd_over_yardstick=(s_size + s_emit) / y,
                 cover_plus_view_rd_over_yardstick=(s_cov + s_size + s_emit) / y)
        del v, rd, runs
    with open(os.path.join(a.out, "rangedel_probe" + (("_" + a.tag) if a.tag else "") + ".jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
