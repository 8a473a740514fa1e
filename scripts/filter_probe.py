#!/usr/bin/env python3
"""Table bloom filters on the device: what a probe costs, and what it saves.

Inputs: config-2 row blocks (gen_row_blocks: 32 KiB, restart interval 16, 16-B
keys, 100-B values; about 1 Mi KVs at --blocks 4096) decoded on the device; the
filter pbl_bloom_build_host writes for their keys at 10 bits per key (about
1.3 MB: served from L2) and one for --big-keys synthetic 16-B keys (32 Mi: about
40 MB, past L2, served from the Infinity Cache); --queries keys that are all
members, all non-members (a member with its last bit flipped), and half and
half.

Arms, each a device-event window over repeated launches after a warm-up, the
arms of one comparison alternating inside one repeat, --repeats repeats:
  a  pbl_filter_probe (named by one filter), small and big filter; with
     --variant LIB the same call into a second build of the library, labelled
     --variant-name (e.g. one built with -DPBL_FILTER_WIDE_LINE=0: loads of the
     probed bytes instead of the whole line)
  b  pbl_seek_batch, table mode: what answering a negative costs without a filter
  c  pbl_seek_prefix_batch: the fused launch
  d  pbl_filter_probe_host, single-threaded (a host clock)
  e  filter.get over 8 small tables with keys of one of them, with and without
     the filter, each run on freshly opened tables so that the decodes it skips
     count (a host clock around work that ends in a synchronise)
The device's answers are compared with the host's before any rate is
reported.  One JSON line per measurement, printed and written to
<out>/filter_probe.jsonl.

  python scripts/filter_probe.py --out profiles/filter
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pebble_amd import _native as N  # noqa: E402
from pebble_amd import filter as F  # noqa: E402
from pebble_amd.batch import BlockBatch, decode  # noqa: E402
from pebble_amd.rowblk import gen_row_blocks  # noqa: E402
from pebble_amd.seek import prepare  # noqa: E402


def timed(fn, min_seconds=0.1, warmup=2):
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


def build_filter(keys16: np.ndarray) -> np.ndarray:
    """pbl_bloom_build_host over an [n, 16] uint8 array of keys, 10 bits per key."""
    L = N.lib()
    n = keys16.shape[0]
    kb = np.ascontiguousarray(keys16).reshape(-1)
    ko = np.arange(0, 16 * (n + 1), 16, dtype=np.uint64)
    cap = int(L.pbl_bloom_build_bound(n, 10))
    out = np.zeros(cap + 16, np.uint8)
    ln = ctypes.c_uint64(0)
    rc = L.pbl_bloom_build_host(kb.ctypes.data, ko.ctypes.data, n, N.PBL_CMP_DEFAULT, 10, out.ctypes.data, cap,
                                ctypes.byref(ln))
    assert rc == 0
    return out[: ln.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--big-keys", type=int, default=32 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--variant", default="", help="a second build of the library for arm a")
    ap.add_argument("--default-name", default="default", help="label of the in-tree build in arm a's lines")
    ap.add_argument("--variant-name", default="variant")
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--table-keys", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join("profiles", "filter"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_probe.py needs a GPU: it measures nothing without one")
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(os.path.join(a.out, "filter_probe.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")

    L = N.lib()
    libs = {a.default_name: L}
    if a.variant:
        V = ctypes.CDLL(os.path.abspath(a.variant))
        V.pbl_filter_probe.restype, V.pbl_filter_probe.argtypes = N.SIGNATURES["pbl_filter_probe"]
        libs[a.variant_name] = V
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- inputs ---------------------------------------------------------------------------
    buf, off, lens, n_kv = gen_row_blocks(2, a.blocks, 32768, 16, 16, 100)
    d = decode(BlockBatch.from_host(buf, off, lens, "cuda", N.PBL_FMT_ROW, 0), entry_off=False, restarts=False)
    t = d.read_totals()
    assert t.status_mask == 0 and int(t.key_bytes) == 16 * n_kv
    members = d.key_bytes[: 16 * n_kv].view(-1, 16)
    small = build_filter(members.cpu().numpy())
    big_keys = np.zeros((a.big_keys, 16), np.uint8)
    big_keys[:, :8] = np.arange(a.big_keys, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(-1, 8)
    big_keys[:, 8:] = np.frombuffer(b"pebble!!", np.uint8)
    big = build_filter(big_keys)
    emit(what="input", n_kv=n_kv, queries=a.queries, small_filter_bytes=int(small.size), big_filter_bytes=int(big.size),
         big_keys=a.big_keys, device=torch.cuda.get_device_name())

    n = a.queries
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    ko = torch.arange(0, 16 * (n + 1), 16, dtype=torch.int64, device="cuda")

    def key_set(src, kind):
        idx = torch.randint(0, src.shape[0], (n,), device="cuda", generator=g)
        k = src[idx].clone()
        if kind == "none":
            k[:, 15] ^= 1
        elif kind == "half":
            k[1::2, 15] ^= 1
        kb = torch.zeros(16 * n + 16, dtype=torch.uint8, device="cuda")
        kb[: 16 * n] = k.view(-1)
        return kb

    big_members = torch.from_numpy(big_keys[: 1 << 22]).cuda()
    del big_keys
    filters = {"small": (torch.from_numpy(np.concatenate([small, np.zeros(16, np.uint8)])).cuda(), small, members),
               "big": (torch.from_numpy(np.concatenate([big, np.zeros(16, np.uint8)])).cuda(), big, big_members)}
    may = torch.empty(n, dtype=torch.uint8, device="cuda")
    which = torch.zeros(n, dtype=torch.int32, device="cuda")

    # ---- a: the probe, d: the host probe ---------------------------------------------------
    for fname, (fdev, fhost, src) in filters.items():
        foff = torch.tensor([0, fhost.size], dtype=torch.int64, device="cuda")
        fs = N.FilterSetC(fdev.data_ptr(), foff.data_ptr(), 1)
        fo = N.FilterOutC(may.data_ptr(), None, None)
        for kind in ("all", "none", "half"):
            kb = key_set(src, kind)
            q = N.FilterQueriesC(kb.data_ptr(), ko.data_ptr(), which.data_ptr(), n, N.PBL_CMP_DEFAULT)

            def run(lib):
                rc = lib.pbl_filter_probe(ctypes.byref(fs), ctypes.byref(q), ctypes.byref(fo), st)
                assert rc == 0

            # the host's answers (arm d), and the device's against them
            hkb = kb.cpu().numpy()
            hko = ko.cpu().numpy().view(np.uint64)
            hoff = np.array([0, fhost.size], np.uint64)
            hmay = np.zeros(n, np.uint8)
            hs = N.FilterSetC(fhost.ctypes.data, hoff.ctypes.data, 1)
            hq = N.FilterQueriesC(hkb.ctypes.data, hko.ctypes.data, None, n, N.PBL_CMP_DEFAULT)
            hout = N.FilterOutC(hmay.ctypes.data, None, None)
            for r in range(min(a.repeats, 3)):
                t0 = time.perf_counter()
                rc = L.pbl_filter_probe_host(ctypes.byref(hs), ctypes.byref(hq), ctypes.byref(hout))
                s = time.perf_counter() - t0
                assert rc == 0
                emit(what="d_host_probe", filter=fname, keys=kind, seconds=s, lines_per_s=n / s, window=r, threads=1)
            for name, lib in libs.items():
                may.zero_()
                run(lib)
                torch.cuda.synchronize()
                assert np.array_equal(may.cpu().numpy(), hmay), (fname, kind, name)
            emit(what="check", filter=fname, keys=kind, equal_to_host=True, may=int(hmay.sum()))
            for r in range(a.repeats):
                for name, lib in libs.items():
                    s, reps = timed(lambda: run(lib))
                    emit(what="a_probe", build=name, filter=fname, keys=kind, seconds=s, lines_per_s=n / s, reps=reps,
                         window=r)
        flush()

    # ---- b: pbl_seek_batch, c: pbl_seek_prefix_batch ------------------------------------------
    idx = prepare(d, N.PBL_CMP_DEFAULT)
    ws = idx.workspace
    o = d.c_struct()
    fdev, fhost, _ = filters["small"]
    kv = torch.empty(n, dtype=torch.int64, device="cuda")
    kv2 = torch.empty(n, dtype=torch.int64, device="cuda")
    ob = torch.empty(n, dtype=torch.int32, device="cuda")
    fl = torch.empty(n, dtype=torch.uint8, device="cuda")
    fl2 = torch.empty(n, dtype=torch.uint8, device="cuda")
    for kind in ("all", "none", "half"):
        kb = key_set(members, kind)
        q = N.SeekQueriesC(kb.data_ptr(), ko.data_ptr(), None, n, N.PBL_CMP_DEFAULT, N.PBL_SEEK_GE, 0)
        out_b = N.SeekOutC(kv.data_ptr(), ob.data_ptr(), fl.data_ptr())
        out_c = N.SeekOutC(kv2.data_ptr(), ob.data_ptr(), fl2.data_ptr())

        def seek_b():
            rc = L.pbl_seek_batch(ctypes.byref(o), d.n_blocks, ctypes.byref(q), ctypes.byref(out_b),
                                  ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
            assert rc == 0

        def seek_c():
            rc = L.pbl_seek_prefix_batch(ctypes.byref(o), d.n_blocks, ctypes.byref(q),
                                         ctypes.c_void_p(fdev.data_ptr()), int(fhost.size), ctypes.byref(out_c),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
            assert rc == 0

        seek_b()
        seek_c()
        torch.cuda.synchronize()
        out = (fl2 & N.PBL_SEEK_FILTERED) != 0
        assert bool((kv2[~out] == kv[~out]).all()) and bool((fl2[~out] == fl[~out]).all())
        assert not bool((out & ((fl & N.PBL_SEEK_EXACT) != 0)).any())
        emit(what="check", arm="c", keys=kind, filtered=int(out.sum().item()),
             exact=int(((fl & N.PBL_SEEK_EXACT) != 0).sum().item()))
        for r in range(a.repeats):
            for name, fn in (("b_seek", seek_b), ("c_seek_prefix", seek_c)):
                s, reps = timed(fn)
                emit(what=name, keys=kind, seconds=s, qps=n / s, reps=reps, window=r)
    flush()

    # ---- e: filter.get over tables, with and without the filter ------------------------------
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import filterutil as FU  # noqa: E402  (the table builder of the tests)
    from pebble_amd.sstable import Table  # noqa: E402
    template = open(os.path.join(ROOT, "tests", "golden", "sst", "h_bloom_no_compression.sst"), "rb").read()
    raw = [FU.bloom_table(template, [b"t%02d_%08d" % (i, j) for j in range(a.table_keys)], per_block=250)
           for i in range(a.tables)]
    keys = [b"t03_%08d" % ((j * 7919) % a.table_keys) for j in range(min(n, 1 << 16))]
    ref = None
    for r in range(a.repeats + 1):  # (the first pass warms both paths and is not reported)
        for use in (True, False):
            tabs = [Table(x) for x in raw]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = F.get(tabs, keys, use_filter=use)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            if ref is None:
                ref = torch.as_tensor(res).clone()
            assert torch.equal(torch.as_tensor(res), ref)
            if r:
                emit(what="e_get", use_filter=use, tables=a.tables, table_keys=a.table_keys, keys=len(keys), seconds=s,
                     n_searched_tables=res.n_searched_tables, n_candidate_pairs=res.n_candidate_pairs, window=r - 1)
    flush()


if __name__ == "__main__":
    main()
