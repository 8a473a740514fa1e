#!/usr/bin/env python3
"""Snapshot-visible view on the device: times of pbl_visible_size / pbl_visible_batch.

Input (merge_probe.py's): --blocks config-2 row blocks
(gen_row_blocks: 32 KiB, restart interval 16, 16-B keys, 100-B values) decoded on
the device.  Every fourth key becomes a user key with four versions, one per
run of K = 4 (run r holds version r, sequence number 4 - r), by the user key's
index modulo 3: SET over SET, DEL over three SETs, MERGE x3 over SET.  The runs
are encoded as row blocks again (256 KVs per block), decoded, scanned and merged
on the device:

  whole   one unbounded range: the visible view of four whole tables' merge
  ranges  --ranges ranges of about 16 user keys

Per case: pbl_visible_size, pbl_visible_batch with PBL_VISIBLE_SIZED, and
pbl_visible_batch alone, each a device-event window over repeated launches after
a warm-up, --repeats windows.  The yardstick runs in the same process before and
after each window: the unchanged pbl_scan_batch (PBL_SCAN_SIZED) with one
unhidden whole-batch query over the generated batch, which holds as many KVs as
the view reads.  Every device result is compared with pbl_visible_batch_host
over to_host() before a time is printed; the to_host() + host time is reported
too (that one measures the host).

The kernels separately: run `--profile` under
  rocprofv3 --output-format csv --kernel-trace -d DIR -o trace -- python scripts/visible_probe.py --profile ...
then `--summarize DIR/.../trace_kernel_trace.csv`, which attributes every
kernel to its case (the grid of visible_bases_kernel) and prints the mean.

One JSON line per measurement, printed and written to <out>/visible_probe.jsonl.

  python scripts/visible_probe.py --blocks 16384 --out profiles/visible
"""
import argparse
import collections
import csv
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
from merge_probe import ARRAYS, Yardstick, encode_run, host_kvs, timed  # noqa: E402
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.merge import merge  # noqa: E402
from pebble_amd.scan import scan  # noqa: E402
from pebble_amd.visible import visible_host  # noqa: E402

D = N.PBL_CMP_DEFAULT
K = 4
SET, MERGE, DEL = 1, 2, 0
KINDS = ((SET, SET, SET, SET), (DEL, SET, SET, SET), (MERGE, MERGE, MERGE, SET))  # newest first, by user key % 3


class Visible:
    """One input batch: sized once, outputs allocated exactly."""

    def __init__(self, batch, snapshot=N.PBL_SEQNUM_MAX):
        self.L, self.batch_in = N.lib(), batch
        self.nb = batch.n_blocks
        self.n_kv = int(batch.read_totals().n_kv)
        self.vin = N.VisibleInC(batch.c_struct(), self.nb, D, self.n_kv, snapshot)
        self.ws = torch.empty(int(self.L.pbl_visible_workspace_bytes(self.nb, self.n_kv)), dtype=torch.uint8, device="cuda")
        self.wp = ctypes.c_void_p(self.ws.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.sized = DecodedBatch.allocate(self.nb, Capacity(0, 0, 0, 0), "cuda", entry_off=False, restarts=False)
        self.so = N.VisibleOutC(self.sized.c_struct(), None, None)
        self.size()
        torch.cuda.synchronize()
        t = self.sized.read_totals()
        self.cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), 0)
        self.out = DecodedBatch.allocate(self.nb, self.cap, "cuda", entry_off=False, restarts=False)
        self.src_kv = torch.empty(max(self.cap.kv, 1), dtype=torch.int64, device="cuda")
        self.n_src = torch.empty(max(self.cap.kv, 1), dtype=torch.int32, device="cuda")
        self.oo = N.VisibleOutC(self.out.c_struct(), self.src_kv.data_ptr(), self.n_src.data_ptr())

    def size(self):
        assert self.L.pbl_visible_size(ctypes.byref(self.vin), ctypes.byref(self.so), self.wp, self.ws.numel(), 0, self.st) == 0

    def batch(self, flags):
        assert self.L.pbl_visible_batch(ctypes.byref(self.vin), ctypes.byref(self.oo), self.wp, self.ws.numel(), flags,
                                        self.st) == 0

    def emit(self):  # the statuses, sizes and roles of the last size()
        self.batch(N.PBL_VISIBLE_SIZED)

    def whole(self):
        self.batch(0)

    def same_as_host(self, hres):
        r, src_kv, n_src = hres
        h = self.out.to_host()
        ok = h["n_kv"] == r["n_kv"] and h["status_mask"] == r["status_mask"]
        for k in ARRAYS + ("kv_flags",):
            ok = ok and np.array_equal(np.asarray(h[k]).astype(np.uint64), np.asarray(r[k]).astype(np.uint64))
        ok = ok and np.array_equal(self.src_kv[: self.cap.kv].cpu().numpy().view(np.uint64), src_kv)
        ok = ok and np.array_equal(self.n_src[: self.cap.kv].cpu().numpy().view(np.uint32), n_src)
        return bool(ok)


def summarize(path):
    """Mean ns per visible kernel, per case, from a rocprofv3 --kernel-trace CSV."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    case = None
    acc = collections.defaultdict(list)
    pending = []  # the kernels of a size pass, which run before the visible_bases_kernel that names their case
    for r in rows:
        name = r["Kernel_Name"]
        if "pbl::visible::" not in name:
            continue
        short = name.split("pbl::visible::")[1].split("(")[0].split("<")[0]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if short not in ("visible_bases_kernel", "visible_heads_kernel", "visible_values_kernel"):
            pending.append((short, ns))
            continue
        if short == "visible_bases_kernel":
            case = "whole" if int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) <= 1 else "ranges"
            for ps, pn in pending:
                acc[(case, ps)].append(pn)
            pending = []
        acc[(case, short)].append(ns)
    return [{"what": "kernel", "case": c, "kernel": s, "calls": len(v), "mean_ns": sum(v) / len(v), "min_ns": min(v),
             "max_ns": max(v)} for (c, s), v in sorted(acc.items(), key=str)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--profile", action="store_true", help="three launches per case, no timing (for a kernel trace)")
    ap.add_argument("--summarize", default="", help="a rocprofv3 kernel trace CSV of a --profile run")
    ap.add_argument("--out", default=os.path.join("profiles", "visible"))
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

    def save(name):
        with open(os.path.join(a.out, name + (("_" + a.tag) if a.tag else "") + ".jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")

    if a.summarize:
        for r in summarize(a.summarize):
            emit(**r)
        save("visible_kernels")
        return
    if not torch.cuda.is_available():
        raise SystemExit("visible_probe.py needs a GPU: it measures nothing without one")

    buf, off, lens, n_gen = gen_blocks(a.blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    t = d.read_totals()
    n_gen_kv = int(t.n_kv)
    assert t.status_mask == 0 and n_gen_kv == n_gen
    keys, _, vals = host_kvs(d.to_host())
    n_user = n_gen_kv // K
    n_kv = n_user * K
    emit(what="input", generated_kvs=n_gen_kv, user_keys=n_user, source_kvs=n_kv, device=torch.cuda.get_device_name())
    yard = Yardstick(d)

    t0 = time.perf_counter()
    tables = []
    ukeys = keys[0:n_kv:K]
    for r in range(K):
        trailers = [(K - r) << 8 | KINDS[u % 3][r] for u in range(n_user)]
        blocks = encode_run(ukeys, trailers, vals[r:n_kv:K])
        tables.append(decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0)))
    emit(what="dealt", runs=K, encode_decode_seconds=time.perf_counter() - t0, blocks_per_run=[x.n_blocks for x in tables])
    n_ranges = max(1, min(a.ranges, n_user // 16))
    at = [16 * i for i in range(n_ranges + 1)]
    cases = (("whole", [None], [None]),
             ("ranges", [ukeys[i] if i else None for i in at[:-1]], [ukeys[i] if i < n_user else None for i in at[1:]]))
    for case, lo, up in cases:
        merged = merge([scan(x, lo, up, comparer=D).batch for x in tables], comparer=D).batch
        covered = n_user if case == "whole" or at[-1] >= n_user else at[-1]  # user keys inside the ranges
        src = int(merged.read_totals().n_kv)
        assert src == K * covered
        v = Visible(merged)
        v.whole()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = merged.to_host()
        to_host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        hres = visible_host(host, comparer=D)
        host_s = time.perf_counter() - t0
        ok = v.same_as_host(hres)
        # two of three user keys survive; a third of those hold four values
        expect = covered - (covered + 1) // 3
        emit(what="check", case=case, ranges=len(lo), equal_to_host=ok, source_kvs=src, result_kvs=v.cap.kv,
             expected_result_kvs=expect, result_val_bytes=v.cap.val, to_host_seconds=to_host_s, host_visible_seconds=host_s,
             host_threads=1, workspace_bytes=v.ws.numel())
        assert ok and v.cap.kv == expect
        del host, hres
        if a.profile:
            for _ in range(3):
                v.size()
                v.emit()
            torch.cuda.synchronize()
            del v, merged
            continue
        for r in range(a.repeats):  # scan / visible / scan
            y0, _ = timed(yard.run)
            s_size, _ = timed(v.size)
            s_emit, reps = timed(v.emit)
            s_whole, _ = timed(v.whole)
            y1, _ = timed(yard.run)
            y = min(y0, y1)
            emit(what="visible", case=case, ranges=len(lo), window=r, size_seconds=s_size, sized_batch_seconds=s_emit,
                 batch_seconds=s_whole, reps=reps, scan_seconds=y0, scan_again_seconds=y1, source_kvs=src,
                 result_kvs=v.cap.kv, scan_kvs=n_gen_kv, ns_per_source_kv=(s_size + s_emit) / src * 1e9,
                 scan_ns_per_kv=y / n_gen_kv * 1e9, per_source_kv_over_scan=((s_size + s_emit) / src) / (y / n_gen_kv),
                 batch_per_source_kv_over_scan=(s_whole / src) / (y / n_gen_kv))
        del v, merged
    save("visible_profile_run" if a.profile else "visible_probe")


def gen_blocks(n):
    from pebble_amd.rowblk import gen_row_blocks
    return gen_row_blocks(2, n, 32768, 16, 16, 100)


if __name__ == "__main__":
    main()
