#!/usr/bin/env python3
"""Columnar keyspan blocks on the device: times of pbl_keyspan_size +
pbl_keyspan_decode.

Input: T disjoint range-deletion fragments over 16-byte keys, one key each,
random sequence numbers, for T = 16, 1 Ki and 64 Ki, as ONE keyspan block and
spread evenly over 16 blocks (pebble_amd.keyspan.Writer).

Per shape: pbl_keyspan_size + pbl_keyspan_decode into exactly sized buffers, a
device-event window over repeated launches after a warm-up, --repeats windows;
also the size call alone and the decode alone (what the emit stage adds).  The
yardsticks run in the same process before and after every window: the row path
over the same fragments as row-format range-del blocks (restart interval 1,
pbl_decode_batch: past 511 entries one wave walks a block serially), and a
device copy of the keyspan block bytes.  Before a time is printed the device
result is compared with pbl_keyspan_decode_host on every array.

One JSON line per measurement, printed and written to <out>/keyspan_probe.jsonl.

  python scripts/keyspan_probe.py --out profiles/keyspan
"""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from merge_probe import timed  # noqa: E402
from pebble_amd import _native as N  # noqa: E402
from pebble_amd import keyspan as K  # noqa: E402
from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode, decode_into  # noqa: E402
from pebble_amd.rowblk import Writer as RowWriter  # noqa: E402

ARRAYS = ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status", "trailer", "kv_flags", "entry_off",
          "key_off", "val_off", "key_bytes", "val_bytes")


def fragments(t, seed=1):
    rng = random.Random(seed)
    return [(b"k%015d" % (2 * f), rng.randrange(1, 1 << 40) << 8 | 15, b"k%015d" % (2 * f + 1)) for f in range(t)]


def keyspan_block(frags) -> bytes:
    w = K.Writer()
    for s, t, e in frags:
        w.add_span(s, e, [(t, b"", b"")])
    return w.finish()


def row_block(frags) -> bytes:
    w = RowWriter(1)
    for s, t, e in frags:
        w.add(s, t, e)
    return w.finish()


class Keyspan:
    """pbl_keyspan_size + pbl_keyspan_decode over preallocated, exactly sized buffers."""

    def __init__(self, blocks):
        self.bb = BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_COL_DEFAULT, 0)
        self.st = torch.cuda.current_stream()
        self.tb = K.total_boundaries(self.bb)
        self.ws = K._workspace(self.bb, self.tb, self.st)
        sz = K.size(self.bb)
        cap = Capacity(sz["n_kv"], sz["key_bytes"], sz["val_bytes"], 0)
        nb = self.bb.n_blocks
        self.sized = DecodedBatch.allocate(nb, Capacity(0, 0, 0, 0), "cuda", entry_off=False, restarts=False)
        self.out = DecodedBatch.allocate(nb, cap, "cuda", entry_off=True, restarts=False)

    def size(self):
        K._run(self.bb, self.sized, None, self.ws, self.tb, self.st, True)

    def decode(self):
        K._run(self.bb, self.out, None, self.ws, self.tb, self.st, False)

    def both(self):
        self.size()
        self.decode()


class Row:
    """The row path: pbl_decode_batch of the row-format range-del blocks."""

    def __init__(self, blocks):
        self.bb = BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0)
        t = decode(self.bb).read_totals()
        cap = Capacity(int(t.n_kv), int(t.key_bytes), int(t.val_bytes), int(t.n_restarts))
        self.out = DecodedBatch.allocate(self.bb.n_blocks, cap, "cuda", max_block_len=self.bb.max_block_len)

    def run(self):
        decode_into(self.bb, self.out)


def windows(fn, yard, repeats):
    """`repeats` windows of fn, every yardstick timed before and after each."""
    out, ys = [], {k: [] for k in yard}
    for _ in range(repeats):
        for k, y in yard.items():
            ys[k].append(timed(y)[0])
        out.append(timed(fn)[0])
        for k, y in yard.items():
            ys[k].append(timed(y)[0])
    return out, ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/keyspan")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="16,1024,65536")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    lines = []
    for t in [int(x) for x in a.sizes.split(",")]:
        frags = fragments(t)
        for nb in (1, 16):
            if t < nb:
                continue
            parts = [frags[q * t // nb: (q + 1) * t // nb] for q in range(nb)]
            blocks = [keyspan_block(p) for p in parts]
            ks, row = Keyspan(blocks), Row([row_block(p) for p in parts])
            # the result before any time
            ks.both()
            torch.cuda.synchronize()
            got, want = ks.out.to_host(), K.decode_host(blocks)
            for k in ARRAYS:
                assert np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)), k
            assert got["n_kv"] == t and got["status_mask"] == 0
            rh = row.out
            row.run()
            torch.cuda.synchronize()
            assert rh.read_totals().n_kv == t and rh.read_totals().status_mask == 0
            src = ks.bb.blocks
            dst = torch.empty_like(src)
            yard = {"row_decode": row.run, "copy": lambda: dst.copy_(src)}
            both, ys = windows(ks.both, yard, a.repeats)
            size_only = [timed(ks.size)[0] for _ in range(a.repeats)]
            decode_only = [timed(ks.decode)[0] for _ in range(a.repeats)]
            us = lambda xs: [round(x * 1e6, 2) for x in xs]  # noqa: E731
            line = {"probe": "keyspan", "fragments": t, "blocks": nb, "block_bytes": int(sum(len(b) for b in blocks)),
                    "row_block_bytes": int(row.bb.input_bytes()), "size_plus_decode_us": us(both),
                    "size_us": us(size_only), "decode_us": us(decode_only), "row_decode_us": us(ys["row_decode"]),
                    "copy_us": us(ys["copy"]), "device": torch.cuda.get_device_name(0)}
            line["ratio_row_over_keyspan"] = round(float(np.median(ys["row_decode"]) / np.median(both)), 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
    with open(os.path.join(a.out, "keyspan_probe.jsonl"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
