#!/usr/bin/env python3
"""Batched k-way merge on the device: times of pbl_merge_size / pbl_merge_batch.

Input: --blocks config-2 row blocks (gen_row_blocks: 32 KiB, restart interval
16, 16-B keys, 100-B values) decoded on the device.  For K in --runs the KVs are
dealt round-robin into K runs, each run encoded as row blocks again (256 KVs
per block), decoded on the device and scanned:

  whole   one unbounded range per run: the merge of K whole tables
  ranges  --ranges ranges of about 16 KVs per run (bounds at every 16 K-th key
          of the undealt batch), the same ranges in every run

Per case: pbl_merge_size, pbl_merge_batch with PBL_MERGE_SIZED, and
pbl_merge_batch alone, each a device-event window over repeated launches after
a warm-up, --repeats windows.  The yardstick runs in the same process between
the merge windows: the unchanged pbl_scan_batch (PBL_SCAN_SIZED) with one
unhidden whole-batch query over the undealt batch, which moves the same bytes.
Every device result is compared with pbl_merge_batch_host over to_host() before
a time is printed, and the whole case also with that scan of the undealt batch;
the to_host() + host merge time is reported too (that one measures the host).

The rank and emit kernels separately: run `--profile` under
  rocprofv3 --output-format csv --kernel-trace -d DIR -o trace -- python scripts/merge_probe.py --profile ...
then `--summarize DIR/.../trace_kernel_trace.csv`, which attributes every merge
kernel to its case (the grid of merge_bases_kernel) and its K (the grid of
merge_rank_kernel) and prints the mean per kernel.

One JSON line per measurement, printed and written to <out>/merge_probe.jsonl.

  python scripts/merge_probe.py --blocks 16384 --out profiles/merge
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.merge import merge_host  # noqa: E402
from pebble_amd.rowblk import Writer, gen_row_blocks  # noqa: E402
from pebble_amd.scan import prepare, scan  # noqa: E402

D = N.PBL_CMP_DEFAULT
ARRAYS = ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_status", "trailer", "key_off", "val_off", "key_bytes",
          "val_bytes")


def timed(fn, min_seconds=0.2, warmup=2):
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
        if s >= min_seconds or reps >= 1 << 14:
            return s / reps, reps
        reps = min(1 << 14, max(reps * 2, int(reps * min_seconds / max(s, 1e-6)) + 1))


def host_kvs(h):
    """(keys, trailers, values) of every KV of a to_host() dict, in batch order."""
    nb = len(h["blk_status"])
    cnt = np.diff(h["blk_kv_base"]).astype(np.int64)
    blk = np.repeat(np.arange(nb), cnt)
    at = np.arange(h["n_kv"]) + blk
    k0 = h["blk_key_base"][blk].astype(np.int64) + h["key_off"][at]
    k1 = h["blk_key_base"][blk].astype(np.int64) + h["key_off"][at + 1]
    v0 = h["blk_val_base"][blk].astype(np.int64) + h["val_off"][at]
    v1 = h["blk_val_base"][blk].astype(np.int64) + h["val_off"][at + 1]
    kb, vb = h["key_bytes"].tobytes(), h["val_bytes"].tobytes()
    return ([kb[a:b] for a, b in zip(k0.tolist(), k1.tolist())], h["trailer"].tolist(),
            [vb[a:b] for a, b in zip(v0.tolist(), v1.tolist())])


def encode_run(keys, trailers, vals, per_block=256):
    w = Writer(16)
    blocks = []
    for i in range(len(keys)):
        w.add(keys[i], trailers[i], vals[i])
        if (i + 1) % per_block == 0:
            blocks.append(w.finish())
            w.reset()
    if len(keys) % per_block:
        blocks.append(w.finish())
    return blocks


class Merge:
    """One set of runs: sized once, outputs allocated exactly."""

    def __init__(self, runs):
        self.L, self.runs = N.lib(), runs
        self.nb = runs[0].n_blocks
        self.n_kv = sum(int(r.read_totals().n_kv) for r in runs)
        self.structs = (N.DecodeOutC * len(runs))(*[r.c_struct() for r in runs])
        self.rs = N.MergeRunsC(ctypes.cast(self.structs, ctypes.POINTER(N.DecodeOutC)), len(runs), self.nb, D, 0,
                               self.n_kv)
        self.ws = torch.empty(int(self.L.pbl_merge_workspace_bytes(len(runs), self.nb, self.n_kv)), dtype=torch.uint8,
                              device="cuda")
        self.wp = ctypes.c_void_p(self.ws.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.sized = DecodedBatch.allocate(self.nb, Capacity(0, 0, 0, 0), "cuda", entry_off=False, restarts=False)
        self.so = N.MergeOutC(self.sized.c_struct(), None, None)
        self.size()
        torch.cuda.synchronize()
        t = self.sized.read_totals()
        self.cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), 0)
        self.out = DecodedBatch.allocate(self.nb, self.cap, "cuda", entry_off=False, restarts=False)
        self.src_run = torch.empty(max(self.cap.kv, 1), dtype=torch.uint8, device="cuda")
        self.src_kv = torch.empty(max(self.cap.kv, 1), dtype=torch.int64, device="cuda")
        self.oo = N.MergeOutC(self.out.c_struct(), self.src_run.data_ptr(), self.src_kv.data_ptr())

    def size(self):
        assert self.L.pbl_merge_size(ctypes.byref(self.rs), ctypes.byref(self.so), self.wp, self.ws.numel(), self.st) == 0

    def batch(self, flags):
        assert self.L.pbl_merge_batch(ctypes.byref(self.rs), ctypes.byref(self.oo), self.wp, self.ws.numel(), flags,
                                      self.st) == 0

    def emit(self):  # the statuses and sizes of the last size()
        self.batch(N.PBL_MERGE_SIZED)

    def whole(self):
        self.batch(0)

    def same_as_host(self, hres):
        r, src_run, src_kv = hres
        h = self.out.to_host()
        ok = h["n_kv"] == r["n_kv"] and h["status_mask"] == r["status_mask"]
        for k in ARRAYS + ("kv_flags",):
            ok = ok and np.array_equal(np.asarray(h[k]).astype(np.uint64), np.asarray(r[k]).astype(np.uint64))
        ok = ok and np.array_equal(self.src_run[: self.cap.kv].cpu().numpy(), src_run)
        ok = ok and np.array_equal(self.src_kv[: self.cap.kv].cpu().numpy().view(np.uint64), src_kv)
        return bool(ok), h


class Yardstick:
    """pbl_scan_batch (PBL_SCAN_SIZED) with one unhidden whole-batch query over the undealt batch."""

    def __init__(self, d):
        self.L, self.d = N.lib(), d
        self.idx = prepare(d, D, False, 1)
        z = torch.zeros(32, dtype=torch.uint8, device="cuda")
        o = torch.zeros(2, dtype=torch.int64, device="cuda")
        fl = torch.full((1,), N.PBL_SCAN_NO_UPPER, dtype=torch.uint8, device="cuda")
        self.keep = (z, o, fl)
        self.q = N.ScanQueriesC(z.data_ptr(), o.data_ptr(), z.data_ptr(), o.data_ptr(), fl.data_ptr(), None, 1, D, 0, 0)
        self.src = d.c_struct()
        self.ws = ctypes.c_void_p(self.idx.workspace.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        t = d.read_totals()
        self.out = DecodedBatch.allocate(1, Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), 0), "cuda",
                                         entry_off=False, restarts=False)
        self.oo = N.ScanOutC(self.out.c_struct(), None, None)
        self.run(0)  # the size pass of this query, left in the workspace
        torch.cuda.synchronize()
        assert int(self.out.read_totals().n_kv) == int(t.n_kv)

    def run(self, flags=N.PBL_SCAN_SIZED):
        assert self.L.pbl_scan_batch(ctypes.byref(self.src), self.d.n_blocks, self.idx.n_kv, ctypes.byref(self.q),
                                     ctypes.byref(self.oo), self.ws, self.idx.workspace.numel(), flags, self.st) == 0


def summarize(path):
    """Mean ns per merge kernel, per (case, K), from a rocprofv3 --kernel-trace CSV."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    case, k = None, None
    acc = collections.defaultdict(list)
    pending = []  # the kernels of a size pass, which run before the merge_bases_kernel that names their case
    for r in rows:
        name = r["Kernel_Name"]
        if "pbl::merge::" not in name:
            continue
        short = name.split("pbl::merge::")[1].split("(")[0].split("<")[0]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if short == "merge_validate_kernel" or short == "merge_rank_kernel":
            k = int(r["Grid_Size_Y"])
        if short in ("merge_validate_kernel", "merge_persize_kernel", "merge_sum_kernel"):
            pending.append((k, short, ns))
            continue
        if short == "merge_bases_kernel":
            case = "whole" if int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) <= 1 else "ranges"
            for pk, ps, pn in pending:
                acc[(case, pk, ps)].append(pn)
            pending = []
        acc[(case, k, short)].append(ns)
    return [{"what": "kernel", "case": c, "runs": kk, "kernel": s, "calls": len(v), "mean_ns": sum(v) / len(v),
             "min_ns": min(v), "max_ns": max(v)} for (c, kk, s), v in sorted(acc.items(), key=str)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--runs", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--profile", action="store_true", help="three launches per case and K, no timing (for a kernel trace)")
    ap.add_argument("--summarize", default="", help="a rocprofv3 kernel trace CSV of a --profile run")
    ap.add_argument("--out", default=os.path.join("profiles", "merge"))
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
        save("merge_kernels")
        return
    if not torch.cuda.is_available():
        raise SystemExit("merge_probe.py needs a GPU: it measures nothing without one")

    buf, off, lens, n_gen = gen_row_blocks(2, a.blocks, 32768, 16, 16, 100)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    t = d.read_totals()
    n_kv = int(t.n_kv)
    assert t.status_mask == 0 and n_kv == n_gen
    emit(what="input", n_kv=n_kv, key_bytes=int(t.key_bytes), val_bytes=int(t.val_bytes),
         device=torch.cuda.get_device_name())
    h = d.to_host()
    keys, trailers, vals = host_kvs(h)
    yard = Yardstick(d)
    whole_scan = yard.out.to_host()

    for K in a.runs:
        t0 = time.perf_counter()
        tables = []
        for r in range(K):
            blocks = encode_run(keys[r::K], trailers[r::K], vals[r::K])
            tables.append(decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0)))
        emit(what="dealt", runs=K, encode_decode_seconds=time.perf_counter() - t0,
             blocks_per_run=[x.n_blocks for x in tables])
        n_ranges = max(1, min(a.ranges, n_kv // (16 * K)))
        at = [16 * K * i for i in range(n_ranges + 1)]
        cases = (("whole", [None], [None]),
                 ("ranges", [keys[i] if i else None for i in at[:-1]], [keys[i] if i < n_kv else None for i in at[1:]]))
        for case, lo, up in cases:
            scans = [scan(x, lo, up, comparer=D).batch for x in tables]
            m = Merge(scans)
            m.whole()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hosts = [s.to_host() for s in scans]
            to_host_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            hres = merge_host(hosts, comparer=D)
            host_s = time.perf_counter() - t0
            ok, got = m.same_as_host(hres)
            same_as_scan = None
            if case == "whole":  # the merge of the dealt tables is the undealt table
                same_as_scan = all(np.array_equal(np.asarray(got[k]).astype(np.uint64),
                                                  np.asarray(whole_scan[k]).astype(np.uint64)) for k in ARRAYS)
            emit(what="check", case=case, runs=K, ranges=len(lo), equal_to_host=ok, equal_to_undealt_scan=same_as_scan,
                 result_kvs=m.cap.kv, to_host_seconds=to_host_s, host_merge_seconds=host_s, host_threads=1,
                 workspace_bytes=m.ws.numel())
            assert ok and same_as_scan is not False
            del hosts, hres, got
            if a.profile:
                for _ in range(3):
                    m.size()
                    m.emit()
                torch.cuda.synchronize()
                del m, scans
                continue
            moved = 2 * (m.cap.kv * (8 + 1 + 4 + 4) + m.cap.key + m.cap.val)
            for r in range(a.repeats):  # scan / merge / scan
                y0, _ = timed(yard.run)
                s_size, _ = timed(m.size)
                s_emit, reps = timed(m.emit)
                s_whole, _ = timed(m.whole)
                y1, _ = timed(yard.run)
                y = min(y0, y1)
                emit(what="merge", case=case, runs=K, ranges=len(lo), window=r, size_seconds=s_size,
                     sized_batch_seconds=s_emit, batch_seconds=s_whole, reps=reps, scan_seconds=y0,
                     scan_again_seconds=y1, result_kvs=m.cap.kv, moved_bytes=moved,
                     merge_gib_s=moved / (s_size + s_emit) / 2**30, scan_gib_s=moved / y / 2**30,
                     size_plus_sized_batch_over_scan=(s_size + s_emit) / y, batch_over_scan=s_whole / y,
                     per_kv_over_scan=((s_size + s_emit) / max(m.cap.kv, 1)) / (y / n_kv),
                     scan_result_kvs=n_kv)
            del m, scans
        del tables
    save("merge_profile_run" if a.profile else "merge_probe")


if __name__ == "__main__":
    main()
