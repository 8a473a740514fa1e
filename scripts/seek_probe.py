#!/usr/bin/env python3
"""Batched seeks on the device against the host: rates of pbl_seek_batch.

Input: config-2 row blocks (gen_row_blocks: 32 KiB, restart interval 16, 16-B
keys, 100-B values) decoded on the device.  Queries: uniformly random existing
keys (even queries) and near-misses (odd queries: an existing key with its last
bit flipped), built on the device.  Per-block and table mode at each query
count; pbl_seek_prepare on its own; and, as the baseline a caller has today,
DecodedBatch.to_host() plus pbl_seek_batch_host single-threaded on a sample of
the same queries (that part measures the host, not the device path).  Every
device timing is a device-event window over repeated launches after a warm-up;
the device results of the sample are compared with the host's before any rate
is reported.  One JSON line per measurement, printed and written to
<out>/seek_probe.jsonl.

  python scripts/seek_probe.py --blocks 16384 --out profiles/seek
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, decode  # noqa: E402
from pebble_amd.rowblk import gen_row_blocks  # noqa: E402
from pebble_amd.seek import prepare  # noqa: E402


SORTED = False


def device_queries(d, n, n_kv, seed):
    """(key bytes uint8 [16 n + 16], offsets int64 [n + 1], block int32 [n]) on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    idx = torch.randint(0, n_kv, (n,), device="cuda", generator=g)
    if SORTED:
        idx = torch.sort(idx).values  # the variant "queries pre-sorted by the caller"
    keys = d.key_bytes[: 16 * n_kv].view(-1, 16)[idx].clone()  # every key of this input is 16 B
    keys[1::2, 15] ^= 1  # near-misses
    kb = torch.zeros(16 * n + 16, dtype=torch.uint8, device="cuda")
    kb[: 16 * n] = keys.view(-1)
    ko = torch.arange(0, 16 * (n + 1), 16, dtype=torch.int64, device="cuda")
    blk = (torch.searchsorted(d.blk_kv_base[: d.n_blocks + 1], idx, right=True) - 1).to(torch.int32)
    return kb, ko, blk


def timed(fn, min_seconds=0.3, warmup=3):
    """Seconds per call: device events around `reps` calls, at least min_seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        s = a.elapsed_time(b) / 1e3
        if s >= min_seconds or reps >= 1 << 16:
            return s / reps, reps
        reps = min(1 << 16, max(reps * 2, int(reps * min_seconds / max(s, 1e-6)) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--queries", type=int, nargs="*", default=[1 << 10, 1 << 16, 1 << 20, 1 << 24])
    ap.add_argument("--host-sample", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "seek"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--sorted", action="store_true", help="queries in key order")
    a = ap.parse_args()
    global SORTED
    SORTED = a.sorted
    if not torch.cuda.is_available():
        raise SystemExit("seek_probe.py needs a GPU: it measures nothing without one")
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kw):
        kw["tag"] = a.tag
        kw["blocks"] = a.blocks
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)

    L = N.lib()
    buf, off, lens, n_kv = gen_row_blocks(2, a.blocks, 32768, 16, 16, 100)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0), entry_off=False, restarts=False)
    t = d.read_totals()
    assert t.status_mask == 0 and int(t.n_kv) == n_kv and int(t.key_bytes) == 16 * n_kv
    emit(what="input", n_kv=n_kv, key_bytes=int(t.key_bytes), val_bytes=int(t.val_bytes), device=torch.cuda.get_device_name())
    o = d.c_struct()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- prepare on its own ---------------------------------------------------------
    idx = prepare(d, N.PBL_CMP_DEFAULT)
    ws = idx.workspace

    def do_prepare():
        rc = L.pbl_seek_prepare(ctypes.byref(o), d.n_blocks, N.PBL_CMP_DEFAULT, ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
        assert rc == 0

    for r in range(a.repeats):
        s, reps = timed(do_prepare)
        emit(what="prepare", seconds=s, reps=reps, window=r, workspace_bytes=ws.numel())

    # ---- the host baseline: to_host(), then pbl_seek_batch_host on a sample -----------------
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = d.to_host()
    to_host_s = time.perf_counter() - t0
    emit(what="to_host", seconds=to_host_s,
         bytes=int(sum(v.nbytes for v in h.values() if isinstance(v, np.ndarray))))
    ns = min(a.host_sample, max(a.queries))
    kb, ko, blk = device_queries(d, ns, n_kv, 7)
    hkb, hko, hblk = kb.cpu().numpy(), ko.cpu().numpy().view(np.uint64), blk.cpu().numpy().view(np.uint32)
    ho = N.DecodeOutC()
    for k in ("kv_flags", "key_off", "key_bytes", "blk_kv_base", "blk_key_base", "blk_status"):
        setattr(ho, k, np.ascontiguousarray(h[k]).ctypes.data)
    host = {}
    for mode in ("block", "table"):
        kv, ob, fl = np.empty(ns, np.uint64), np.empty(ns, np.uint32), np.empty(ns, np.uint8)
        q = N.SeekQueriesC(hkb.ctypes.data, hko.ctypes.data, hblk.ctypes.data if mode == "block" else None, ns,
                           N.PBL_CMP_DEFAULT, N.PBL_SEEK_GE, 0)
        out = N.SeekOutC(kv.ctypes.data, ob.ctypes.data, fl.ctypes.data)
        best = None
        for r in range(a.repeats):
            t0 = time.perf_counter()
            rc = L.pbl_seek_batch_host(ctypes.byref(ho), d.n_blocks, ctypes.byref(q), ctypes.byref(out))
            s = time.perf_counter() - t0
            assert rc == 0
            emit(what="host", mode=mode, queries=ns, seconds=s, qps=ns / s, window=r, threads=1)
            best = s if best is None else min(best, s)
        host[mode] = (best, kv.copy(), ob.copy(), fl.copy())

    # ---- the device ----------------------------------------------------------------------
    for n in a.queries:
        same = n == ns  # (the same seed and count: the host sample's queries again)
        kb, ko, blk = device_queries(d, n, n_kv, 7)
        kv = torch.empty(n, dtype=torch.int64, device="cuda")
        ob = torch.empty(n, dtype=torch.int32, device="cuda")
        fl = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = N.SeekOutC(kv.data_ptr(), ob.data_ptr(), fl.data_ptr())
        for mode in ("block", "table"):
            q = N.SeekQueriesC(kb.data_ptr(), ko.data_ptr(), blk.data_ptr() if mode == "block" else None, n,
                               N.PBL_CMP_DEFAULT, N.PBL_SEEK_GE, 0)
            w = ws if mode == "table" else None

            def do_seek():
                rc = L.pbl_seek_batch(ctypes.byref(o), d.n_blocks, ctypes.byref(q), ctypes.byref(out),
                                      ctypes.c_void_p(w.data_ptr()) if w is not None else None,
                                      w.numel() if w is not None else 0, st)
                assert rc == 0

            do_seek()
            torch.cuda.synchronize()
            if same:  # the device's answers are the host's, before any rate is reported
                _, ekv, eob, efl = host[mode]
                assert (kv.cpu().numpy().view(np.uint64) == ekv).all()
                assert (ob.cpu().numpy().view(np.uint32) == eob).all() and (fl.cpu().numpy() == efl).all()
                emit(what="check", mode=mode, queries=n, equal_to_host=True,
                     exact=int((efl & N.PBL_SEEK_EXACT != 0).sum()))
            for r in range(a.repeats):
                s, reps = timed(do_seek)
                line = dict(what="device", mode=mode, queries=n, seconds=s, qps=n / s, reps=reps, window=r)
                if same:
                    line["host_seconds"] = host[mode][0]
                    line["host_plus_to_host_seconds"] = host[mode][0] + to_host_s
                    line["speedup_vs_host"] = host[mode][0] / s
                    line["speedup_vs_host_plus_to_host"] = (host[mode][0] + to_host_s) / s
                emit(**line)
    with open(os.path.join(a.out, "seek_probe%s.jsonl" % (("_" + a.tag) if a.tag else "")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
