#!/usr/bin/env python3
"""Range keys in the device read path: the time of pbl_rangekey_mask against
pbl_rangedel_cover over the same decoded batch, and of the host set builder
(DESIGN.md §3.16).

Input: --blocks config-2 row blocks (scripts/rangedel_probe.py's generator),
their 16-byte keys made user keys under the testkeys comparer: every user key
u has four versions u@4 .. u@1, in one batch of row blocks.  Spans: T fragments
spread evenly over the user keys, each covering half of its stride, dealt to 4
runs, for T = 16, 1 Ki and 4 Ki.  The range-deletion set and the range-key set
are built on the same fragments, so they hold the same boundaries; a range-key
fragment holds m sets (m = 1: the suffix @3, which masks @2 and @1 under the
threshold @9; m = 4: @3 and three older ones).

Per T and m, in one process, parent / variant / parent: pbl_rangedel_cover
(comparer testkeys), pbl_rangekey_mask, pbl_rangedel_cover again, each a
device-event window over repeated launches after a warm-up, --repeats windows.
Before a time is printed the mask is compared with a numpy statement of it
(the fragments are disjoint: a KV is masked iff its user key lies in a fragment
and its version is below 3) and, for T = 16, with pbl_rangekey_mask_host.  The
set builder is the host form: its wall time next to the device time of
pbl_rangedel_set over the same fragments.

One JSON line per measurement, printed and written to <out>/rangekey_probe.jsonl.

  python scripts/rangekey_probe.py --blocks 2048 --out profiles/rangekey
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
from pebble_amd import keyspan, rangekey  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode  # noqa: E402
from pebble_amd.rowblk import Writer  # noqa: E402
from visible_probe import gen_blocks  # noqa: E402

T_CMP = N.PBL_CMP_TESTKEYS
SEQ = 3
VERSIONS = 4


class Cover:
    """pbl_rangedel_set over `runs` and pbl_rangedel_cover of `batch` under the testkeys comparer."""

    def __init__(self, runs, batch):
        self.L = N.lib()
        tots = [r.read_totals() for r in runs]
        self.T = sum(int(t.n_kv) for t in tots)
        self.structs = (N.DecodeOutC * len(runs))(*[r.c_struct() for r in runs])
        self.cnt = (ctypes.c_uint64 * len(runs))(*[int(t.n_kv) for t in tots])
        self.rs = N.RangedelRunsC(ctypes.cast(self.structs, ctypes.POINTER(N.DecodeOutC)),
                                  ctypes.cast(self.cnt, ctypes.POINTER(ctypes.c_uint64)), len(runs), T_CMP, N.PBL_SEQNUM_MAX)
        self.ws = torch.empty(int(self.L.pbl_rangedel_workspace_bytes(self.T)), dtype=torch.uint8, device="cuda")
        cap = Capacity(2 * self.T, sum(int(t.key_bytes) + int(t.val_bytes) for t in tots), 0, 0)
        self.set = DecodedBatch.allocate(1, cap, "cuda", entry_off=False, restarts=False)
        self.sc, self.bc, self.nb = self.set.c_struct(), batch.c_struct(), batch.n_blocks
        self.n_kv = int(batch.read_totals().n_kv)
        self.cover = torch.zeros(max(self.n_kv, 1), dtype=torch.int64, device="cuda")
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.keep = runs

    def build(self):
        assert self.L.pbl_rangedel_set(ctypes.byref(self.rs), ctypes.byref(self.sc), ctypes.c_void_p(self.ws.data_ptr()),
                                       self.ws.numel(), self.st) == 0

    def lookup(self):
        assert self.L.pbl_rangedel_cover(ctypes.byref(self.sc), ctypes.byref(self.bc), self.nb, self.n_kv, T_CMP,
                                         ctypes.c_void_p(self.cover.data_ptr()), self.st) == 0


class Mask:
    """pbl_rangekey_mask of `batch` under a set on the device; outputs allocated once."""

    def __init__(self, set_dev, batch, t: bytes):
        self.L, self.set = N.lib(), set_dev
        self.sc, self.xc, self.bc, self.nb = set_dev.batch.c_struct(), set_dev.extras.c_struct(), batch.c_struct(), batch.n_blocks
        self.n_kv = int(batch.read_totals().n_kv)
        self.cover = torch.zeros(max(self.n_kv, 1), dtype=torch.int64, device="cuda")
        self.t = torch.zeros(len(t) + 16, dtype=torch.uint8, device="cuda")
        self.t[: len(t)] = torch.from_numpy(np.frombuffer(t, np.uint8).copy())
        self.tl = len(t)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(self):
        assert self.L.pbl_rangekey_mask(ctypes.byref(self.sc), ctypes.byref(self.xc), ctypes.byref(self.bc), self.nb,
                                        self.n_kv, T_CMP, ctypes.c_void_p(self.t.data_ptr()), self.tl,
                                        ctypes.c_void_p(self.cover.data_ptr()), self.st) == 0


def rangedel_block(frags):
    w = Writer(1)
    for s, e in frags:
        w.add(s, SEQ << 8 | N.PBL_KIND_RANGEDEL, e)
    return w.finish()


def rangekey_block(frags, m):
    w = keyspan.Writer()
    sfx = [b"@3", b"@2", b"@1", b"@0"][:m]
    for s, e in frags:
        w.add_span(s, e, [((SEQ + m - j) << 8 | N.PBL_KIND_RANGEKEYSET, x, b"v") for j, x in enumerate(sfx)])
    return w.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--fragments", type=int, nargs="*", default=[16, 1 << 10, 1 << 12])
    ap.add_argument("--sets", type=int, nargs="*", default=[1, 4], help="sets per range-key fragment")
    ap.add_argument("--repeats", type=int, default=3, help="independent timing windows per measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "rangekey"))
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
        raise SystemExit("rangekey_probe.py needs a GPU: it measures nothing without one")
    buf, off, lens, _ = gen_blocks(a.blocks)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0))
    keys, _, vals = host_kvs(d.to_host())
    ukeys = sorted({k.replace(b"@", b"?") for k in keys[::VERSIONS]})  # (a user key without the suffix delimiter)
    n_user = len(ukeys)
    pkeys = [u + b"@%d" % v for u in ukeys for v in range(VERSIONS, 0, -1)]
    batch = decode(BlockBatch.from_blocks(encode_run(pkeys, [7 << 8 | 1] * len(pkeys), vals[: len(pkeys)]), "cuda",
                                          N.PBL_FMT_ROW, 0))
    src = int(batch.read_totals().n_kv)
    assert src == len(pkeys)
    emit(what="input", user_keys=n_user, source_kvs=src, device=torch.cuda.get_device_name())
    hu = np.repeat(np.array(ukeys, dtype="S16"), VERSIONS)
    ver = np.tile(np.arange(VERSIONS, 0, -1), n_user)
    hb = batch.to_host()

    for T in a.fragments:
        T = min(T, n_user // 2)
        stride = n_user // T
        frags = [(ukeys[f * stride], ukeys[f * stride + max(1, stride // 2)]) for f in range(T)]
        starts = np.array([f[0] for f in frags], dtype="S16")
        ends = np.array([f[1] for f in frags], dtype="S16")
        at = np.searchsorted(starts, hu, side="right") - 1
        inside = (at >= 0) & (hu < ends[np.maximum(at, 0)])
        rd = Cover([decode(BlockBatch.from_blocks([rangedel_block(frags[r::4])], "cuda", N.PBL_FMT_ROW, 0)) for r in range(4)],
                   batch)
        s_rdset, _ = timed(rd.build)
        rd.lookup()
        torch.cuda.synchronize()
        assert np.array_equal(rd.cover[:src].cpu().numpy() > 0, inside)
        for m in a.sets:
            runs = [keyspan.decode(BlockBatch.from_blocks([rangekey_block(frags[r::4], m)], "cuda", N.PBL_FMT_ROW, 0),
                                   extras=True) for r in range(4)]
            hosts = [r.to_host() for r in runs]
            t0 = time.perf_counter()
            hset = rangekey.build_set_host(hosts, T_CMP)
            host_set_s = time.perf_counter() - t0
            assert hset["status_mask"] == 0 and hset["n_kv"] == T * m
            mk = Mask(rangekey.to_device(hset, "cuda"), batch, b"@9")
            mk.run()
            torch.cuda.synchronize()
            got = mk.cover[:src].cpu().numpy().view(np.uint64)
            want = np.where(inside & (ver < 3), N.PBL_RANGEDEL_ALL, 0).astype(np.uint64)
            ok = bool(np.array_equal(got, want))
            if T <= 16:
                hm, st = rangekey.mask_host(hosts, hb, T_CMP, b"@9")
                ok = ok and st == 0 and bool(np.array_equal(hm, want))
            emit(what="check", fragments=T, sets=m, mask_equal=ok, masked_kvs=int((want > 0).sum()),
                 boundaries=2 * T, set_kvs=int(hset["n_kv"]))
            assert ok
            for w in range(a.repeats):
                c0, _ = timed(rd.lookup)
                s_mask, _ = timed(mk.run)
                c1, _ = timed(rd.lookup)
                emit(what="mask", fragments=T, sets=m, window=w, cover_seconds=c0, mask_seconds=s_mask, cover_again_seconds=c1,
                     source_kvs=src, mask_ns_per_kv=s_mask / src * 1e9, cover_ns_per_kv=min(c0, c1) / src * 1e9,
                     mask_over_cover=s_mask / min(c0, c1), parent_spread=abs(c0 - c1) / min(c0, c1))
            emit(what="set", fragments=T, sets=m, host_set_seconds=host_set_s, rangedel_set_device_seconds=s_rdset,
                 host_over_rangedel_set=host_set_s / s_rdset)
            del mk, runs
        del rd
    with open(os.path.join(a.out, "rangekey_probe" + (("_" + a.tag) if a.tag else "") + ".jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
