#!/usr/bin/env python3
"""Diagnostic: per-phase cycles of rowblk_pool_kernel (PBL_STAMPS build,
PBL_LIB=<diag .so>) on a config-2 batch.  Stamps (rowblk_pool.hip.h): 8 the
wave's loop iteration starts (the end of the emit before), 0 stage acquired +
ticket taken by the loop, 10 the same by the prefetch of the emit before (the
DMA issued), 1 descriptor read, 2 staged (DMA landed), 3 walk + scan + publish,
9 stage released, 4 metadata + value buckets, 5 look-back resolved, 6 keys /
per-KV arrays written, 7 values done; 11-14 are counts of the block's look-back
resolve, not times: round trips (the first included), block records consumed,
cycles in the single-lane poll on an unpublished predecessor, chunk records
consumed (PBL_LB_L2).  A block carries stamp 0 or stamp 10,
whichever way its stage was taken (a workspace reused from an earlier launch
may hold both: the later one counts).  A build from before stamp 9 released
the stage at 4.
Read the shares; the stamps perturb timing."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pebble_amd import _native as N  # noqa: E402
from pebble_amd.batch import BlockBatch, decode  # noqa: E402
from pebble_amd.rowblk import gen_row_blocks  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
wl = os.environ.get("WORKLOAD", "row")  # row (config 2) or zipf:RI (config 5, row format)
if wl.startswith("zipf"):
    from pebble_amd.batch import gen_zipf_blocks
    buf, off, lens, n = gen_zipf_blocks(42, nb, N.PBL_FMT_ROW, int(wl.split(":")[1]), 32768, n_threads=16)
else:
    buf, off, lens, n = gen_row_blocks(42, nb, 32768, 16, 16, 100, n_threads=16)
b = BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, N.PBL_KERNEL_POOL)
for _ in range(3):
    out = decode(b)
    ws_state = 256 + 10 * nb * 8 + 16 * ((nb + 63) // 64)
    out.workspace[ws_state: ws_state + nb * 16 * 8].zero_()  # (the next launch may get this memory again)
out = decode(b)
torch.cuda.synchronize()
ws_state = 256 + 10 * nb * 8 + 16 * ((nb + 63) // 64)
st = out.workspace[ws_state: ws_state + nb * 16 * 8].view(torch.int64).view(nb, 16).cpu().numpy().copy()


def show(nm, d):
    d = d.astype(np.float64)
    if d.size:
        print(f"{nm:34s} median {np.median(d):9.0f} mean {np.mean(d):9.0f} p90 {np.percentile(d, 90):9.0f} cycles"
              f"  ({d.size} blocks)")


phases = [("acquire stage + ticket (loop)", 8, 0), ("descriptor (loop)", 0, 1),
          ("prefetch issued -> emit end", 10, 8), ("stage (DMA wait in the front)", 1, 2),
          ("walk + scan + publish", 2, 3), ("metadata + buckets", 3, 4), ("look-back finish", 4, 5),
          ("keys + values (steps)", 5, 7), ("block total (loop start -> done)", 8, 7)]
for nm, a, z in phases:
    m = (st[:, a] > 0) & (st[:, z] > 0) & (st[:, z] >= st[:, a])
    show(nm, st[m, z] - st[m, a])
# the stage: from whichever acquire happened (prefetch or loop) to the release
acq = np.maximum(st[:, 0], st[:, 10])
rel = np.where(st[:, 9] > 0, st[:, 9], st[:, 4])
m = (acq > 0) & (rel > acq)
show("stage held (acquire -> release)", rel[m] - acq[m])
pre = st[:, 10] > st[:, 0]
print(f"blocks staged by a prefetch: {pre.sum()} of {nb} ({100.0 * pre.mean():.1f} %)")
for nm, sel in (("  stage held, prefetched", m & pre), ("  stage held, loop-acquired", m & ~pre)):
    show(nm, rel[sel] - acq[sel])
# the wave's idle gap: the end of one emit (the loop iteration's start) to the start of the next walk
m = (st[:, 8] > 0) & (st[:, 2] > st[:, 8])
show("idle gap (emit end -> walk start)", st[m, 2] - st[m, 8])
for nm, sel in (("  idle gap, prefetched", m & pre), ("  idle gap, loop-acquired", m & ~pre)):
    show(nm, st[sel, 2] - st[sel, 8])
# the look-back resolve per block (counts, slots 11-14; the poll in cycles)
lb = st[:, 11] > 0
for nm, col in (("look-back round trips", 11), ("look-back block records consumed", 12),
                ("look-back chunk records consumed", 14), ("look-back poll (unpublished pred.)", 13)):
    d = st[lb, col].astype(np.float64)
    if d.size:
        print(f"{nm:34s} median {np.median(d):9.1f} mean {np.mean(d):9.2f} p90 {np.percentile(d, 90):9.1f}"
              f"  ({d.size} blocks)")
if lb.any():
    trips = st[lb, 11]
    print("round trips per resolve, share of blocks: " +
          ", ".join(f"{k}: {100.0 * (trips == k).mean():.1f} %" for k in range(1, 6)) +
          f", more: {100.0 * (trips > 5).mean():.1f} %;  resolves that polled: {100.0 * (st[lb, 13] > 0).mean():.1f} %")
t0, t7 = st[:, 8][st[:, 8] > 0], st[:, 7][st[:, 7] > 0]
print(f"kernel span {t7.max() - t0.min():.0f} cycles; blocks per CU {nb / 256:.0f}; "
      f"cycles per block per CU {(t7.max() - t0.min()) / (nb / 256):.0f}")
