#!/usr/bin/env python3
"""Compaction view on the device: times of pbl_compact_size / pbl_compact_batch.

Input (visible_probe.py's): --blocks config-2 row blocks decoded
on the device; every fourth key becomes a user key with four versions, one per
run of K = 4, by the user key's index modulo 3: SET over SET, DEL over three
SETs, MERGE x3 over SET.  Odd user keys carry the sequence numbers 4..1, even
ones 14..11.  The runs are encoded as row blocks again, decoded, scanned and
merged on the device, per case

  whole   one unbounded range: four whole tables' merge
  ranges  --ranges ranges of about 16 user keys

and per snapshot list

  none    no snapshots: one stripe
  three   (13, 100, 200): the even user keys split into two stripes of two
          versions each, the odd ones stay in one: half of the keys split

Per combination: pbl_compact_size, pbl_compact_batch with PBL_COMPACT_SIZED, and
pbl_compact_batch alone, each a device-event window over repeated launches after
a warm-up, --repeats windows.  The yardstick runs in the same process before and
after each window: the unchanged pbl_visible_batch (PBL_VISIBLE_SIZED) over the
same merged input; pbl_visible_size and pbl_visible_batch alone are timed in the
same window for the whole-call comparison.  Every device result is compared with
pbl_compact_batch_host over to_host() before a time is printed; the to_host() +
host time is reported too (that one measures the host).

The kernels separately: run `--profile` under
  rocprofv3 --output-format csv --kernel-trace -d DIR -o trace -- python scripts/compact_probe.py --profile ...
then `--summarize DIR/.../trace_kernel_trace.csv`, which attributes every
kernel to its combination (they run in a fixed order, eight compact_bases_kernel
launches each) and prints the mean.

One JSON line per measurement, printed and written to <out>/compact_probe.jsonl.

  python scripts/compact_probe.py --blocks 16384 --out profiles/compact
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
from merge_probe import ARRAYS, encode_run, host_kvs, timed  # noqa: E402
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.compact import compact_host  # noqa: E402
from pebble_amd.merge import merge  # noqa: E402
from pebble_amd.scan import scan  # noqa: E402
from visible_probe import KINDS, Visible, gen_blocks, K  # noqa: E402

D = N.PBL_CMP_DEFAULT
SNAPSHOTS = (("none", ()), ("three", (13, 100, 200)))
COMBOS = [(c, s) for c in ("whole", "ranges") for s, _ in SNAPSHOTS]
BASES_PER_COMBO = 8  # the constructor's size, the checked call, three size + emit pairs


class Compact:
    """One input batch and snapshot list: sized once, outputs allocated exactly."""

    def __init__(self, batch, snapshots, flags=0):
        self.L, self.batch_in, self.flags = N.lib(), batch, flags
        self.nb = batch.n_blocks
        self.n_kv = int(batch.read_totals().n_kv)
        self.snaps = torch.tensor(list(snapshots), dtype=torch.int64, device="cuda") if snapshots else None
        self.cin = N.CompactInC(batch.c_struct(), self.nb, D, self.n_kv,
                                self.snaps.data_ptr() if self.snaps is not None else None, len(snapshots))
        self.ws = torch.empty(int(self.L.pbl_compact_workspace_bytes(self.nb, self.n_kv)), dtype=torch.uint8, device="cuda")
        self.wp = ctypes.c_void_p(self.ws.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.sized = DecodedBatch.allocate(self.nb, Capacity(0, 0, 0, 0), "cuda", entry_off=False, restarts=False)
        self.so = N.CompactOutC(self.sized.c_struct(), None, None, None, None, None, None)
        self.size()
        torch.cuda.synchronize()
        t = self.sized.read_totals()
        self.cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), 0)
        self.out = DecodedBatch.allocate(self.nb, self.cap, "cuda", entry_off=False, restarts=False)
        n = max(self.cap.kv, 1)
        self.src_kv = torch.empty(n, dtype=torch.int64, device="cuda")
        self.n_src = torch.empty(n, dtype=torch.int32, device="cuda")
        self.pinned = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros((3, max(self.nb, 1)), dtype=torch.int32, device="cuda")
        self.oo = N.CompactOutC(self.out.c_struct(), self.src_kv.data_ptr(), self.n_src.data_ptr(), self.pinned.data_ptr(),
                                *[self.counts[i].data_ptr() for i in range(3)])

    def size(self):
        assert self.L.pbl_compact_size(ctypes.byref(self.cin), ctypes.byref(self.so), self.wp, self.ws.numel(), self.flags,
                                       self.st) == 0

    def batch(self, flags):
        assert self.L.pbl_compact_batch(ctypes.byref(self.cin), ctypes.byref(self.oo), self.wp, self.ws.numel(),
                                        self.flags | flags, self.st) == 0

    def emit(self):  # everything the last size() left
        self.batch(N.PBL_COMPACT_SIZED)

    def whole(self):
        self.batch(0)

    def same_as_host(self, hres):
        r = hres["batch"]
        h = self.out.to_host()
        ok = h["n_kv"] == r["n_kv"] and h["status_mask"] == r["status_mask"]
        for k in ARRAYS + ("kv_flags",):
            ok = ok and np.array_equal(np.asarray(h[k]).astype(np.uint64), np.asarray(r[k]).astype(np.uint64))
        n = self.cap.kv
        ok = ok and np.array_equal(self.src_kv[:n].cpu().numpy().view(np.uint64), hres["src_kv"])
        ok = ok and np.array_equal(self.n_src[:n].cpu().numpy().view(np.uint32), hres["n_src"])
        ok = ok and np.array_equal(self.pinned[:n].cpu().numpy(), hres["pinned"])
        for i, k in enumerate(("n_missized", "n_ineffectual", "n_nondeterministic")):
            ok = ok and np.array_equal(self.counts[i][: self.nb].cpu().numpy().view(np.uint32), hres[k])
        return bool(ok)


def summarize(path):
    """Mean ns per compact kernel, per combination, from a rocprofv3 --kernel-trace CSV."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    acc = collections.defaultdict(list)
    pending, bases = [], 0
    for r in rows:
        name = r["Kernel_Name"]
        if "pbl::compact::" not in name:
            continue
        short = name.split("pbl::compact::")[1].split("(")[0].split("<")[0]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if short not in ("compact_bases_kernel", "compact_heads_kernel", "compact_values_kernel"):
            pending.append((short, ns))
            continue
        if short == "compact_bases_kernel":
            combo = COMBOS[min(bases // BASES_PER_COMBO, len(COMBOS) - 1)]
            bases += 1
            for ps, pn in pending:
                acc[(combo, ps)].append(pn)
            pending = []
        acc[(combo, short)].append(ns)
    return [{"what": "kernel", "case": c[0], "snapshots": c[1], "kernel": s, "calls": len(v), "mean_ns": sum(v) / len(v),
             "min_ns": min(v), "max_ns": max(v)} for (c, s), v in sorted(acc.items(), key=str)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--profile", action="store_true", help="three launches per combination, no timing (for a kernel trace)")
    ap.add_argument("--summarize", default="", help="a rocprofv3 kernel trace CSV of a --profile run")
    ap.add_argument("--out", default=os.path.join("profiles", "compact"))
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
        save("compact_kernels")
        return
    if not torch.cuda.is_available():
        raise SystemExit("compact_probe.py needs a GPU: it measures nothing without one")

    buf, off, lens, n_gen = gen_blocks(a.blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    t = d.read_totals()
    n_gen_kv = int(t.n_kv)
    assert t.status_mask == 0 and n_gen_kv == n_gen
    keys, _, vals = host_kvs(d.to_host())
    del d
    n_user = n_gen_kv // K
    n_kv = n_user * K
    emit(what="input", generated_kvs=n_gen_kv, user_keys=n_user, source_kvs=n_kv, device=torch.cuda.get_device_name())

    t0 = time.perf_counter()
    tables = []
    ukeys = keys[0:n_kv:K]
    for r in range(K):
        trailers = [(K - r + (0 if u % 2 else 10)) << 8 | KINDS[u % 3][r] for u in range(n_user)]
        blocks = encode_run(ukeys, trailers, vals[r:n_kv:K])
        tables.append(decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0)))
    emit(what="dealt", runs=K, encode_decode_seconds=time.perf_counter() - t0, blocks_per_run=[x.n_blocks for x in tables])
    n_ranges = max(1, min(a.ranges, n_user // 16))
    at = [16 * i for i in range(n_ranges + 1)]
    cases = {"whole": ([None], [None]),
             "ranges": ([ukeys[i] if i else None for i in at[:-1]], [ukeys[i] if i < n_user else None for i in at[1:]])}
    merged = {c: merge([scan(x, lo, up, comparer=D).batch for x in tables], comparer=D).batch for c, (lo, up) in cases.items()}
    for case, sname in COMBOS:
        snaps = dict(SNAPSHOTS)[sname]
        m = merged[case]
        src = int(m.read_totals().n_kv)
        c = Compact(m, snaps)
        c.whole()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = m.to_host()
        to_host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        hres = compact_host(host, comparer=D, snapshots=snaps)
        host_s = time.perf_counter() - t0
        ok = c.same_as_host(hres)
        emit(what="check", case=case, snapshots=sname, ranges=m.n_blocks, equal_to_host=ok, source_kvs=src, result_kvs=c.cap.kv,
             result_val_bytes=c.cap.val, to_host_seconds=to_host_s, host_compact_seconds=host_s, host_threads=1,
             workspace_bytes=c.ws.numel(), pinned=int(hres["pinned"].sum()))
        assert ok
        del hres, host
        if a.profile:
            for _ in range(3):
                c.size()
                c.emit()
            torch.cuda.synchronize()
            del c
            continue
        v = Visible(m)
        for r in range(a.repeats):  # view / compact / view
            v.size()
            y0, _ = timed(v.emit)
            vs, _ = timed(v.size)
            vw, _ = timed(v.whole)
            s_size, _ = timed(c.size)
            s_emit, reps = timed(c.emit)
            s_whole, _ = timed(c.whole)
            v.size()
            y1, _ = timed(v.emit)
            y = min(y0, y1)
            emit(what="compact", case=case, snapshots=sname, ranges=m.n_blocks, window=r, size_seconds=s_size,
                 sized_batch_seconds=s_emit, batch_seconds=s_whole, reps=reps, view_sized_seconds=y0,
                 view_sized_again_seconds=y1, view_size_seconds=vs, view_batch_seconds=vw, source_kvs=src, result_kvs=c.cap.kv,
                 view_result_kvs=v.cap.kv, size_ns_per_source_kv=s_size / src * 1e9, sized_batch_ns_per_source_kv=s_emit / src * 1e9,
                 batch_ns_per_source_kv=s_whole / src * 1e9, view_sized_ns_per_source_kv=y / src * 1e9,
                 sized_batch_over_view_sized=s_emit / y, size_over_view_sized=s_size / y, batch_over_view_sized=s_whole / y,
                 batch_over_view_batch=s_whole / vw)
        del v, c
    save("compact_profile_run" if a.profile else "compact_probe")


if __name__ == "__main__":
    main()
