#!/usr/bin/env python3
"""Fixture of the columnar keyspan blocks, read as DATA from
the reference's test data (run where the reference checkout is,
make_fixtures.REF; the tests read only the output):

  tests/golden/keyspan.json
      blocks    every block that sstable/colblk/testdata/keyspan_block finishes
                and the two keyspan blocks that
                sstable/testdata/columnar_writer/simple_binary describes (its
                `range-del` and `range-key` layouts): the block's bytes, rebuilt
                from the `NN-MM: x HEX` / `b BITS` lines of its description; the
                spans it was built from (the `add` / `Span:` inputs); and every
                forward walk the file holds over it (an `iter` whose commands
                begin first, next, ... up to the exhausted "."), with its
                synthetic-seq-num when it has one.
                The second keyspan_block build (b-d, e-g) holds a legal gap
                span, [d, e) (asserted below).
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF, parse_datadriven  # noqa: E402

KINDS = {"RANGEDEL": 15, "RANGEKEYDEL": 19, "RANGEKEYUNSET": 20, "RANGEKEYSET": 21}
BYTES = re.compile(r"(\d+)-(\d+): ([xb]) ?([0-9a-f]*)(?:\s+#.*)?$")
SPAN = re.compile(r"^(\S+?)-(\S+?):\{(.*)\}$")
KEY = re.compile(r"\(#(\d+),([A-Z]+)(?:,([^,)]*))?(?:,([^)]*))?\)")


def parse_span(line: str):
    m = SPAN.match(line.strip())
    assert m, line
    keys = [[int(seq), KINDS[kind], suffix or "", value or ""] for seq, kind, suffix, value in KEY.findall(m.group(3))]
    assert keys, line
    return {"start": m.group(1), "end": m.group(2), "keys": keys}


def block_bytes(lines) -> bytes:
    """The bytes a block description's leaf lines spell out."""
    buf = bytearray()
    for ln in lines:
        m = BYTES.search(ln)
        if not m:
            continue
        lo, hi, form, digits = int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)
        raw = bytes.fromhex(digits) if form == "x" else bytes(int(digits[i:i + 8], 2) for i in range(0, len(digits), 8))
        assert lo == len(buf) and hi - lo == len(raw), ln
        buf += raw
    return bytes(buf)


def forward_walk(case):
    """(synthetic_seq_num, [span ...]) of an `iter` that begins first, next, ...
    and runs to the end, else None."""
    args = case["cmd"].split()[1:]
    ssn = 0
    for a in args:
        if not a.startswith("synthetic-seq-num="):
            return None
        ssn = int(a.split("=")[1])
    ops, out = case["input"].split("\n"), case["expected"].split("\n")
    if not ops or ops[0] != "first":
        return None
    spans = []
    for i, (op, line) in enumerate(zip(ops, out)):
        if op != ("first" if i == 0 else "next"):
            return None
        if line == ".":
            return ssn, spans
        spans.append(parse_span(line))
    return None


def keyspan_block_cases():
    path = os.path.join(REF, "sstable", "colblk", "testdata", "keyspan_block")
    blocks, spans, cur = [], [], None
    for c in parse_datadriven(path):
        cmd = c["cmd"].split()[0]
        if cmd in ("init", "reset"):
            spans, cur = [], None
        elif cmd == "add":
            spans += [parse_span(ln) for ln in c["input"].split("\n") if ln.strip()]
        elif cmd == "finish":
            blk = block_bytes(c["expected"].split("\n"))
            cur = {"name": "keyspan_block/%d" % len(blocks), "hex": blk.hex(), "spans": list(spans), "walks": []}
            blocks.append(cur)
        elif cmd == "iter" and cur is not None:
            w = forward_walk(c)
            if w is not None:
                cur["walks"].append({"synthetic_seq_num": w[0], "spans": w[1]})
    return blocks


def simple_binary_cases():
    path = os.path.join(REF, "sstable", "testdata", "columnar_writer", "simple_binary")
    blocks, spans = [], []
    for c in parse_datadriven(path):
        cmd = c["cmd"].split()[0]
        if cmd == "build":
            spans = [parse_span(ln[len("Span:"):]) for ln in c["input"].split("\n") if ln.startswith("Span:")]
        elif cmd == "layout" and spans:
            lines = c["expected"].split("\n")
            for kind in ("range-del", "range-key"):
                at = [i for i, ln in enumerate(lines) if re.search(r"── %s  offset: \d+  length: \d+$" % kind, ln)]
                if not at:
                    continue
                length = int(lines[at[0]].rsplit("length: ", 1)[1])
                end = next(i for i in range(at[0] + 1, len(lines)) if "trailer [compression" in lines[i])
                blk = block_bytes(lines[at[0] + 1: end])
                assert len(blk) == length, (kind, len(blk), length)
                blocks.append({"name": "simple_binary/%s" % kind, "hex": blk.hex(), "spans": spans, "walks": []})
    return blocks


def main():
    blocks = keyspan_block_cases() + simple_binary_cases()
    names = [b["name"] for b in blocks]
    assert names == ["keyspan_block/0", "keyspan_block/1", "keyspan_block/2", "simple_binary/range-del",
                     "simple_binary/range-key"], names
    gap = blocks[2]
    assert [(s["start"], s["end"]) for s in gap["spans"]] == [("b", "d"), ("e", "g")]
    assert any(w["synthetic_seq_num"] == 99 for w in gap["walks"]) and blocks[0]["walks"]
    for b in blocks:
        assert int.from_bytes(bytes.fromhex(b["hex"])[:4], "little") >= 2, b["name"]
    out = os.path.join(HERE, "keyspan.json")
    with open(out, "w") as f:
        json.dump({"source": ["sstable/colblk/testdata/keyspan_block", "sstable/testdata/columnar_writer/simple_binary"],
                   "kinds": KINDS, "blocks": blocks}, f, indent=1)
        f.write("\n")
    print(out, len(blocks), "blocks", sum(len(b["walks"]) for b in blocks), "walks")


if __name__ == "__main__":
    main()
