#!/usr/bin/env python3
"""Row-block encoder on the device: times of pbl_rowenc_size / pbl_rowenc_batch.

Input (compact_probe.py's): --blocks config-2 row blocks dealt
into four runs, decoded, scanned, merged and compacted on the device, per case

  whole   one unbounded range: one stream
  ranges  --ranges ranges of about 16 user keys: many short streams

The compaction's result is encoded with restart interval 16, threshold 90 and
target 4 KiB and 32 KiB.  Per combination: pbl_rowenc_size, pbl_rowenc_batch
with PBL_ROWENC_SIZED, and pbl_rowenc_batch alone, each a device-event window
over repeated launches after a warm-up, --repeats windows.  The yardsticks run
in the same windows:

  copy    a device copy of the output bytes (the floor of any emit)
  decode  the row decode of the blocks just written (the sibling)
  host    to_host() of the input and pbl_rowenc_batch_host over it, one thread
          (what a caller has without the device form; measured once)

Every device result is compared with the host form before a time is printed.

The stages separately: run `--profile` under
  rocprofv3 --output-format csv --kernel-trace -d DIR -o trace -- python scripts/rowenc_probe.py --profile ...
then `--summarize DIR/.../trace_kernel_trace.csv`: the trace is cut into the
calls that launched the kernels, and per combination and kind of call (size,
sized emit, call alone; three of each after the constructor's size and the
checked call, which are left out) the mean time per kernel, per stage
(describe / partition / emit) and of all kernels of one call is printed.

One JSON line per measurement, printed and written to <out>/rowenc_probe.jsonl.

  python scripts/rowenc_probe.py --blocks 16384 --out profiles/rowenc
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
from merge_probe import encode_run, host_kvs, timed  # noqa: E402
from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, decode, decode_into  # noqa: E402
from pebble_amd.compact import compact  # noqa: E402
from pebble_amd.merge import merge  # noqa: E402
from pebble_amd.rowenc import RowEncOptions, encode_host  # noqa: E402
from pebble_amd.scan import scan  # noqa: E402
from visible_probe import KINDS, gen_blocks, K  # noqa: E402

D = N.PBL_CMP_DEFAULT
TARGETS = (4096, 32768)
COMBOS = [(c, t) for c in ("whole", "ranges") for t in TARGETS]
STAGES = {"describe": ("rowenc_classify_kernel", "rowenc_obs_tiles_kernel", "rowenc_describe_kernel", "rowenc_dsum_kernel",
                       "rowenc_tile_scan_kernel", "rowenc_prefix_kernel"),
          "partition": ("rowenc_next_kernel", "rowenc_round_kernel", "rowenc_mark_sum_kernel", "rowenc_mark_scan_kernel",
                        "rowenc_blocks_kernel", "rowenc_streams_kernel"),
          "emit": ("rowenc_emit_kernel",)}
CALLS_PER_COMBO = 11  # the constructor's size, the checked call, three times (size, sized emit, call alone)
WARM_CALLS = 2        # of which the first two are left out of the means
RERUN = ("rowenc_blocks_kernel", "rowenc_streams_kernel")  # what a sized call runs again before it emits


class Encode:
    """One input batch and option set: sized once, outputs allocated exactly."""

    def __init__(self, batch, opts):
        self.L, self.batch_in, self.opts = N.lib(), batch, opts
        self.nb = batch.n_blocks
        self.n_kv = int(batch.read_totals().n_kv)
        self.cin = N.RowEncInC(batch.c_struct(), self.nb, 0, self.n_kv)
        self.co = opts.c_struct()
        u = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device="cuda")  # noqa: E731
        self.ws = u(self.L.pbl_rowenc_workspace_bytes(self.nb, self.n_kv), torch.uint8)
        self.wp = ctypes.c_void_p(self.ws.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.totals = torch.zeros(ctypes.sizeof(N.RowEncTotalsC), dtype=torch.uint8, device="cuda")
        self.sbb, self.sst = u(self.nb + 1, torch.int64), u(self.nb, torch.int32)
        self.so = N.RowEncOutC(None, None, None, None, None, None, self.sbb.data_ptr(), self.sst.data_ptr(), None,
                               self.totals.data_ptr(), 0, 0)
        self.size()
        torch.cuda.synchronize()
        t = self.read_totals()
        self.n_blocks, self.block_bytes = int(t.n_blocks), int(t.block_bytes)
        self.blocks, self.copy_dst = u(self.block_bytes, torch.uint8), u(self.block_bytes, torch.uint8)
        self.off, self.first = u(self.n_blocks, torch.int64), u(self.n_blocks, torch.int64)
        self.len, self.bst, self.nkv = (u(self.n_blocks, torch.int32) for _ in range(3))
        self.obs = u(self.n_kv, torch.uint8)
        self.oo = N.RowEncOutC(self.blocks.data_ptr(), self.off.data_ptr(), self.len.data_ptr(), self.bst.data_ptr(),
                               self.first.data_ptr(), self.nkv.data_ptr(), self.sbb.data_ptr(), self.sst.data_ptr(),
                               self.obs.data_ptr(), self.totals.data_ptr(), self.block_bytes, self.n_blocks)

    def read_totals(self):
        return N.RowEncTotalsC.from_buffer_copy(self.totals.cpu().numpy().tobytes())

    def size(self):
        assert self.L.pbl_rowenc_size(ctypes.byref(self.cin), ctypes.byref(self.co), ctypes.byref(self.so), self.wp,
                                      self.ws.numel(), self.st) == 0

    def batch(self, flags):
        assert self.L.pbl_rowenc_batch(ctypes.byref(self.cin), ctypes.byref(self.co), ctypes.byref(self.oo), self.wp,
                                       self.ws.numel(), flags, self.st) == 0

    def emit(self):  # the partition the last size() left
        self.batch(N.PBL_ROWENC_SIZED)

    def whole(self):
        self.batch(0)

    def copy(self):
        self.copy_dst.copy_(self.blocks)

    def block_batch(self):
        return BlockBatch(self.blocks, self.off, self.len, N.PBL_FMT_ROW, self.opts.decode_flags(),
                          max_block_len=int(self.len.max().item()) if self.n_blocks else 0)

    def same_as_host(self, h):
        g = lambda x, dt: x.cpu().numpy().view(dt)  # noqa: E731
        t = self.read_totals()
        ok = (int(t.n_blocks), int(t.block_bytes), int(t.n_restarts), int(t.status_mask)) == (
            h["n_blocks"], h["block_bytes"], h["n_restarts"], h["status_mask"])
        for k, x, dt in (("blocks", self.blocks, np.uint8), ("block_off", self.off, np.uint64),
                         ("block_len", self.len, np.uint32), ("block_stream", self.bst, np.uint32),
                         ("block_first_kv", self.first, np.uint64), ("block_n_kv", self.nkv, np.uint32),
                         ("stream_block_base", self.sbb, np.uint64), ("obsolete", self.obs, np.uint8)):
            ok = ok and np.array_equal(g(x, dt)[: len(h[k])], h[k])
        return bool(ok)


def calls_of(rows):
    """The encoder kernels of a trace, in time order, cut into the calls that launched them: a call starts
    at the classify kernel (pbl_rowenc_size; pbl_rowenc_batch alone when it ends in the emit), or, for a
    sized pbl_rowenc_batch, at the blocks kernel that follows a call's last kernel."""
    calls = []
    for r in rows:
        name = r["Kernel_Name"]
        if "pbl::rowenc::" not in name:
            continue
        short = name.split("pbl::rowenc::")[1].split("(")[0].split("<")[0]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        last = calls[-1][-1][0] if calls else ""
        if short == "rowenc_classify_kernel" or (short == "rowenc_blocks_kernel" and last in ("rowenc_streams_kernel",
                                                                                               "rowenc_emit_kernel")):
            calls.append([])
        calls[-1].append((short, ns))
    out = []
    for c in calls:
        names = [n for n, _ in c]
        kind = ("batch" if names[-1] == "rowenc_emit_kernel" else "size") if names[0] == "rowenc_classify_kernel" else "sized"
        per = collections.defaultdict(int)
        for n, ns in c:
            per[n] += ns  # (the doubling rounds of one call add up)
        out.append((kind, per))
    return out


def summarize(path):
    """Mean ns per kernel and per stage of one call, per combination and kind of call (size: pbl_rowenc_size;
    sized: pbl_rowenc_batch with PBL_ROWENC_SIZED, whose 'partition' is the rerun of the last scan pass;
    batch: pbl_rowenc_batch alone), from a rocprofv3 --kernel-trace CSV of a --profile run."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls = calls_of(rows)
    assert len(calls) == CALLS_PER_COMBO * len(COMBOS), (len(calls), [k for k, _ in calls])
    acc = collections.defaultdict(list)
    for at, (kind, per) in enumerate(calls):
        combo, nth = COMBOS[at // CALLS_PER_COMBO], at % CALLS_PER_COMBO
        assert kind == (("size", "batch") + ("size", "sized", "batch") * 3)[nth], (at, kind)
        if nth < WARM_CALLS:
            continue
        for n, ns in per.items():
            acc[(combo, kind, n)].append(ns)
        for stage, names in STAGES.items():
            acc[(combo, kind, "stage:" + stage)].append(sum(per.get(n, 0) for n in names))
        acc[(combo, kind, "all kernels")].append(sum(per.values()))
    return [{"what": "kernel", "case": c[0], "target": c[1], "call": kind, "kernel": s, "calls": len(v),
             "mean_ns": sum(v) / len(v), "min_ns": min(v), "max_ns": max(v)}
            for (c, kind, s), v in sorted(acc.items(), key=str)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--ranges", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--profile", action="store_true", help="three launches per combination, no timing (for a kernel trace)")
    ap.add_argument("--summarize", default="", help="a rocprofv3 kernel trace CSV of a --profile run")
    ap.add_argument("--out", default=os.path.join("profiles", "rowenc"))
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
        save("rowenc_kernels")
        return
    if not torch.cuda.is_available():
        raise SystemExit("rowenc_probe.py needs a GPU: it measures nothing without one")

    buf, off, lens, n_gen = gen_blocks(a.blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    n_gen_kv = int(d.read_totals().n_kv)
    keys, _, vals = host_kvs(d.to_host())
    del d
    n_user = n_gen_kv // K
    n_kv = n_user * K
    tables = []
    ukeys = keys[0:n_kv:K]
    for r in range(K):
        trailers = [(K - r + (0 if u % 2 else 10)) << 8 | KINDS[u % 3][r] for u in range(n_user)]
        tables.append(decode(BlockBatch.from_blocks(encode_run(ukeys, trailers, vals[r:n_kv:K]), "cuda", N.PBL_FMT_ROW, 0)))
    n_ranges = max(1, min(a.ranges, n_user // 16))
    at = [16 * i for i in range(n_ranges + 1)]
    cases = {"whole": ([None], [None]),
             "ranges": ([ukeys[i] if i else None for i in at[:-1]], [ukeys[i] if i < n_user else None for i in at[1:]])}
    kept = {}
    for c, (lo, up) in cases.items():
        m = merge([scan(x, lo, up, comparer=D).batch for x in tables], comparer=D).batch
        kept[c] = compact(m, comparer=D).batch
        del m
    emit(what="input", generated_kvs=n_gen_kv, user_keys=n_user, device=torch.cuda.get_device_name(),
         kept_kvs={c: int(b.read_totals().n_kv) for c, b in kept.items()})
    hosts = {}
    for case, target in COMBOS:
        opts = RowEncOptions(16, target, 90, D)
        b = kept[case]
        src = int(b.read_totals().n_kv)
        e = Encode(b, opts)
        e.whole()
        torch.cuda.synchronize()
        if case not in hosts:
            t0 = time.perf_counter()
            hosts[case] = (b.to_host(), time.perf_counter() - t0)
        host, to_host_s = hosts[case]
        t0 = time.perf_counter()
        h = encode_host(host, opts)  # (runs the loop twice: sizes, then bytes)
        host_s = (time.perf_counter() - t0) / 2
        ok = e.same_as_host(h)
        emit(what="check", case=case, target=target, streams=b.n_blocks, equal_to_host=ok, source_kvs=src,
             n_blocks=e.n_blocks, block_bytes=e.block_bytes, to_host_seconds=to_host_s, host_encode_seconds=host_s,
             host_threads=1, workspace_bytes=e.ws.numel())
        assert ok
        del h
        if a.profile:
            for _ in range(3):
                e.size()
                e.emit()
                e.whole()
            torch.cuda.synchronize()
            del e
            continue
        bb = e.block_batch()
        dout = decode(bb, exact=True)  # exact capacities, reused by every timed decode
        dec = lambda: decode_into(bb, dout)  # noqa: E731
        for r in range(a.repeats):  # copy / encode / copy
            e.size()
            y0, _ = timed(e.copy)
            s_size, _ = timed(e.size)
            s_emit, reps = timed(e.emit)
            s_whole, _ = timed(e.whole)
            y1, _ = timed(e.copy)
            s_dec, _ = timed(dec)
            y = min(y0, y1)
            gib = e.block_bytes / 2 ** 30
            emit(what="encode", case=case, target=target, streams=b.n_blocks, window=r, size_seconds=s_size,
                 sized_batch_seconds=s_emit, batch_seconds=s_whole, reps=reps, copy_seconds=y0, copy_again_seconds=y1,
                 decode_seconds=s_dec, source_kvs=src, n_blocks=e.n_blocks, block_bytes=e.block_bytes,
                 batch_gib_per_s=gib / s_whole, sized_batch_gib_per_s=gib / s_emit, copy_gib_per_s=gib / y,
                 batch_ns_per_kv=s_whole / src * 1e9, sized_batch_over_copy=s_emit / y, batch_over_copy=s_whole / y,
                 batch_over_decode=s_whole / s_dec, host_over_batch=host_s / s_whole)
        del e, bb, dout
    save("rowenc_profile_run" if a.profile else "rowenc_probe")


if __name__ == "__main__":
    main()
