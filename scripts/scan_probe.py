#!/usr/bin/env python3
"""Batched bounded scans on the device: rates of pbl_scan_size / pbl_scan_batch.

Input: config-2 row blocks (gen_row_blocks: 32 KiB, restart interval 16, 16-B
keys, 100-B values, every --obsolete-every'th KV an obsolete point) decoded on
the device.  Three measurements:

  whole   one query over the whole batch with HideObsoletePoints, next to
          pbl_transform_batch with HideObsoletePoints alone over the same batch
          in the same process (the same compaction, the same bytes moved);
          their outputs are compared array by array before any rate
  ranges  --queries random ranges of about --lengths KVs: size and emit times,
          result KVs/s, GB/s of bytes read plus written; the baseline a caller
          has today, DecodedBatch.to_host() plus pbl_scan_batch_host single-
          threaded, on a sample of the same queries (that part measures the host)
  copy    one unhidden query over the whole batch next to a torch
          device-to-device copy of the same number of bytes

Every device timing is a device-event window over repeated launches after a
warm-up; device results are compared with the host's before a rate is
reported.  One JSON line per measurement, printed and written to
<out>/scan_probe.jsonl.

  python scripts/scan_probe.py --blocks 16384 --out profiles/scan
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
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.rowblk import gen_row_blocks  # noqa: E402
from pebble_amd.scan import prepare, scan_host  # noqa: E402
from pebble_amd.transforms import TransformPlan, Transforms  # noqa: E402

D = N.PBL_CMP_DEFAULT


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


class Scan:
    """One query set over decoded batch d: sized once, outputs allocated exactly."""

    def __init__(self, d, idx, lb, lo, ub, uo, fl, hide):
        self.L, self.d, self.idx = N.lib(), d, idx
        self.keep = (lb, lo, ub, uo, fl)
        self.n = int(lo.numel()) - 1
        self.q = N.ScanQueriesC(lb.data_ptr(), lo.data_ptr(), ub.data_ptr(), uo.data_ptr(),
                                fl.data_ptr() if fl is not None else None, None, self.n, D, 1 if hide else 0, 0)
        self.src = d.c_struct()
        self.ws = ctypes.c_void_p(idx.workspace.data_ptr())
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.rng = torch.empty((self.n, 2), dtype=torch.int64, device="cuda")
        self.sized = DecodedBatch.allocate(self.n, Capacity(0, 0, 0, 0), "cuda", entry_off=False, restarts=False)
        self.so = N.ScanOutC(self.sized.c_struct(), self.rng.data_ptr(), None)
        self.size()
        torch.cuda.synchronize()
        t = self.sized.read_totals()
        self.cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), 0)
        self.out = DecodedBatch.allocate(self.n, self.cap, "cuda", entry_off=False, restarts=False)
        self.src_kv = torch.empty(max(self.cap.kv, 1), dtype=torch.int64, device="cuda")
        self.oo = N.ScanOutC(self.out.c_struct(), self.rng.data_ptr(), self.src_kv.data_ptr())
        # per result KV: trailer, flags, two offsets, the source index; its key and value bytes
        self.out_bytes = self.cap.kv * (8 + 1 + 4 + 4 + 8) + self.cap.key + self.cap.val
        self.in_bytes = self.cap.kv * (8 + 1 + 4 + 4) + self.cap.key + self.cap.val

    def size(self):
        rc = self.L.pbl_scan_size(ctypes.byref(self.src), self.d.n_blocks, self.idx.n_kv, ctypes.byref(self.q),
                                  ctypes.byref(self.so), self.ws, self.idx.workspace.numel(), self.st)
        assert rc == 0

    def batch(self, flags):
        rc = self.L.pbl_scan_batch(ctypes.byref(self.src), self.d.n_blocks, self.idx.n_kv, ctypes.byref(self.q),
                                   ctypes.byref(self.oo), self.ws, self.idx.workspace.numel(), flags, self.st)
        assert rc == 0

    def emit(self):  # the bounds of the last size()
        self.batch(N.PBL_SCAN_SIZED)

    def whole(self):  # searches, sizes and emit
        self.batch(0)


def dev_bounds(keys16, lo_idx, hi_idx, n_kv):
    """Bounds [key[lo], key[hi]) as device arrays (every key of this input is 16 B);
    hi == n_kv: PBL_SCAN_NO_UPPER."""
    n = int(lo_idx.numel())

    def pack(idx):
        kb = torch.zeros(16 * n + 16, dtype=torch.uint8, device="cuda")
        kb[: 16 * n] = keys16[idx.clamp(max=n_kv - 1)].reshape(-1)
        return kb

    off = torch.arange(0, 16 * (n + 1), 16, dtype=torch.int64, device="cuda")
    fl = (hi_idx >= n_kv).to(torch.uint8) * N.PBL_SCAN_NO_UPPER
    return pack(lo_idx), off, pack(hi_idx), off.clone(), fl


def host_bounds(b):
    lb, lo, ub, uo, fl = (x.cpu().numpy() for x in b)
    n = len(lo) - 1
    lows = [lb[16 * i: 16 * i + 16].tobytes() for i in range(n)]
    ups = [None if fl[i] else ub[16 * i: 16 * i + 16].tobytes() for i in range(n)]
    return lows, ups


def same_as_host(sc, hres):
    """The device result of `sc` equals scan_host's, array by array."""
    r, rng, src = hres
    t = sc.out.read_totals()
    ok = (int(t.n_kv), int(t.key_bytes), int(t.val_bytes), int(t.status_mask)) == \
        (r["n_kv"], r["key_bytes_total"], r["val_bytes_total"], r["status_mask"])
    h = sc.out.to_host()
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_status", "trailer", "kv_flags", "key_off", "val_off",
              "key_bytes", "val_bytes"):
        ok = ok and np.array_equal(np.asarray(h[k]).astype(np.uint64), np.asarray(r[k]).astype(np.uint64))
    ok = ok and np.array_equal(sc.rng.cpu().numpy().view(np.uint64), rng)
    ok = ok and np.array_equal(sc.src_kv[: sc.cap.kv].cpu().numpy().view(np.uint64), src)
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--obsolete-every", type=int, default=4)
    ap.add_argument("--queries", type=int, nargs="*", default=[1 << 10, 1 << 16, 1 << 20])
    ap.add_argument("--lengths", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--host-kvs", type=int, default=1 << 22, help="result KVs of the host baseline's sample, at most")
    ap.add_argument("--max-out-gib", type=float, default=16.0, help="skip a ranges case whose result is larger")
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--only", choices=["whole", "ranges", "copy"], nargs="*", default=["whole", "ranges", "copy"])
    ap.add_argument("--out", default=os.path.join("profiles", "scan"))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_probe.py needs a GPU: it measures nothing without one")
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kw):
        kw["tag"] = a.tag
        kw["blocks"] = a.blocks
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)

    buf, off, lens, n_gen = gen_row_blocks(2, a.blocks, 32768, 16, 16, 100, obsolete_every=a.obsolete_every)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    t = d.read_totals()
    n_kv = int(t.n_kv)
    assert t.status_mask == 0 and n_kv == n_gen and int(t.key_bytes) == 16 * n_kv
    emit(what="input", n_kv=n_kv, key_bytes=int(t.key_bytes), val_bytes=int(t.val_bytes),
         obsolete_every=a.obsolete_every, device=torch.cuda.get_device_name())
    keys16 = d.key_bytes[: 16 * n_kv].view(-1, 16)
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    whole_bounds = dev_bounds(keys16, z, z + n_kv, n_kv)
    whole_bounds = (whole_bounds[0], torch.zeros(2, dtype=torch.int64, device="cuda")) + whole_bounds[2:]  # First()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = d.to_host()
    to_host_s = time.perf_counter() - t0
    emit(what="to_host", seconds=to_host_s, bytes=int(sum(v.nbytes for v in h.values() if isinstance(v, np.ndarray))))

    for hide, name in ((True, "whole"), (False, "copy")):
        if name not in a.only:
            continue
        idx = prepare(d, D, hide, 1)
        o = d.c_struct()
        ws = idx.workspace

        def do_prepare():
            rc = N.lib().pbl_scan_prepare(ctypes.byref(o), d.n_blocks, n_kv, D, 1 if hide else 0,
                                          ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0

        for r in range(a.repeats):
            s, reps = timed(do_prepare)
            emit(what="prepare", hide=hide, seconds=s, reps=reps, window=r, workspace_bytes=ws.numel())
        sc = Scan(d, idx, *whole_bounds, hide)
        sc.whole()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hres = scan_host(h, [None], [None], comparer=D, hide_obsolete_points=hide)
        host_s = time.perf_counter() - t0
        emit(what="check", case=name, equal_to_host=same_as_host(sc, hres), result_kvs=sc.cap.kv, host_seconds=host_s)
        assert lines and json.loads(lines[-1])["equal_to_host"]
        moved = sc.in_bytes + sc.out_bytes
        if hide:
            # the transform pass with HideObsoletePoints alone: the same compaction
            plan = TransformPlan(d, Transforms(hide_obsolete_points=True))
            plan.launch()
            torch.cuda.synchronize()
            tt = plan.out.read_totals()
            same = (int(tt.n_kv), int(tt.key_bytes), int(tt.val_bytes)) == (sc.cap.kv, sc.cap.key, sc.cap.val)
            for x, y, n in ((plan.out.trailer, sc.out.trailer, sc.cap.kv), (plan.out.kv_flags, sc.out.kv_flags, sc.cap.kv),
                            (plan.out.key_bytes, sc.out.key_bytes, sc.cap.key),
                            (plan.out.val_bytes, sc.out.val_bytes, sc.cap.val)):
                same = same and bool(torch.equal(x[:n], y[:n]))
            emit(what="check", case="whole vs transform", equal=same)
            assert same
            for r in range(a.repeats):  # transform / scan / transform
                s0, _ = timed(plan.launch)
                s1, reps = timed(sc.emit)
                s2, _ = timed(sc.whole)
                s3, _ = timed(plan.launch)
                emit(what="whole", window=r, transform_seconds=s0, transform_again_seconds=s3, emit_seconds=s1,
                     scan_batch_seconds=s2, reps=reps, result_kvs=sc.cap.kv, moved_bytes=moved,
                     emit_gib_s=moved / s1 / 2**30, transform_gib_s=moved / min(s0, s3) / 2**30,
                     emit_over_transform=s1 / min(s0, s3))
        else:
            src_t = torch.empty(sc.out_bytes, dtype=torch.uint8, device="cuda")
            dst_t = torch.empty_like(src_t)
            for r in range(a.repeats):
                s0, _ = timed(lambda: dst_t.copy_(src_t))
                s1, reps = timed(sc.emit)
                s2, _ = timed(lambda: dst_t.copy_(src_t))
                emit(what="copy", window=r, emit_seconds=s1, d2d_seconds=s0, d2d_again_seconds=s2, reps=reps,
                     bytes=sc.out_bytes, emit_gib_s=2 * sc.out_bytes / s1 / 2**30,
                     d2d_gib_s=2 * sc.out_bytes / min(s0, s2) / 2**30, emit_over_d2d=s1 / min(s0, s2))
            del src_t, dst_t
        del sc

    if "ranges" in a.only:
        g = torch.Generator(device="cuda")
        for hide in (False, True):
            for ln in a.lengths:
                for n in a.queries:
                    if n * ln * 150 > a.max_out_gib * 2**30:
                        emit(what="ranges", hide=hide, queries=n, length=ln, skipped="result larger than --max-out-gib")
                        continue
                    g.manual_seed(7 + ln)
                    lo_i = torch.randint(0, n_kv, (n,), device="cuda", generator=g)
                    jit = torch.randint(ln - ln // 4, ln + ln // 4 + 1, (n,), device="cuda", generator=g)
                    b = dev_bounds(keys16, lo_i, lo_i + jit, n_kv)
                    idx = prepare(d, D, hide, n)
                    sc = Scan(d, idx, *b, hide)
                    sc.emit()
                    torch.cuda.synchronize()
                    ns = max(1, min(n, a.host_kvs // ln))
                    sb = tuple(x[: 16 * ns + 16] if i in (0, 2) else x[: ns + 1] if i in (1, 3) else x[:ns]
                               for i, x in enumerate(b))
                    lows, ups = host_bounds(sb)
                    t0 = time.perf_counter()
                    hres = scan_host(h, lows, ups, comparer=D, hide_obsolete_points=hide)
                    host_s = time.perf_counter() - t0
                    ss = Scan(d, idx, *sb, hide)
                    ss.emit()
                    torch.cuda.synchronize()
                    ok = same_as_host(ss, hres)
                    emit(what="check", case="ranges", hide=hide, queries=ns, length=ln, equal_to_host=ok)
                    assert ok
                    s_dev, _ = timed(lambda: (ss.size(), ss.emit()))
                    emit(what="host", hide=hide, queries=ns, length=ln, host_seconds=host_s, to_host_seconds=to_host_s,
                         result_kvs=ss.cap.kv, device_seconds=s_dev, speedup_vs_host=host_s / s_dev,
                         speedup_vs_host_plus_to_host=(host_s + to_host_s) / s_dev, threads=1)
                    del ss
                    sc.size()
                    for r in range(a.repeats):
                        s_size, _ = timed(sc.size)
                        s_emit, reps = timed(sc.emit)
                        tot = s_size + s_emit
                        emit(what="ranges", hide=hide, queries=n, length=ln, window=r, size_seconds=s_size,
                             emit_seconds=s_emit, reps=reps, result_kvs=sc.cap.kv, kvs_per_s=sc.cap.kv / tot,
                             gb_s=(sc.in_bytes + sc.out_bytes) / tot / 1e9)
                    del sc, idx
    with open(os.path.join(a.out, "scan_probe%s.jsonl" % (("_" + a.tag) if a.tag else "")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
