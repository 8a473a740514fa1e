#!/usr/bin/env python3
"""Fixture of the row-block encoder, read as DATA from the
reference's sstable/testdata/writer_v3 (run where the reference checkout is,
make_fixtures.REF; the tests read only the output):

  tests/golden/rowenc.json
      the `build ... block-size=1 index-block-size=1` cases that are followed
      by a `layout` command: their table format (absent = the default format
      of the test, where a SET's value carries a prefix byte), their KVs
      (`key#seq,KIND:value` lines) and the lengths of the `data` lines of the
      layout, in order.
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF, parse_datadriven  # noqa: E402

KINDS = {"DEL": 0, "SET": 1, "MERGE": 2, "SINGLEDEL": 7, "SETWITHDEL": 18, "DELSIZED": 23}
LINE = re.compile(r"^([^#\s]+)#(\d+),([A-Z]+):(.*)$")
DATA = re.compile(r"data\s+offset:\s*(\d+)\s+length:\s*(\d+)")


def main() -> None:
    cases = parse_datadriven(os.path.join(REF, "sstable", "testdata", "writer_v3"))
    out = []
    for c, nxt in zip(cases, cases[1:]):
        words = c["cmd"].split()
        if words[0] != "build" or "block-size=1" not in words or nxt["cmd"].strip() != "layout":
            continue
        kvs = []
        for line in c["input"].split("\n"):
            m = LINE.match(line.strip())
            if not m:
                kvs = None
                break
            kvs.append({"key": m.group(1), "seq": int(m.group(2)), "kind": KINDS[m.group(3)], "value": m.group(4)})
        if not kvs:
            continue
        fmt = [w.split("=", 1)[1] for w in words if w.startswith("table-format=")]
        out.append({"cmd": c["cmd"], "table_format": fmt[0] if fmt else None, "kvs": kvs,
                    "data_block_lengths": [int(m.group(2)) for m in DATA.finditer(nxt["expected"])]})
    assert out, "no case found"
    with open(os.path.join(HERE, "rowenc.json"), "w") as f:
        json.dump({"source": "sstable/testdata/writer_v3", "cases": out}, f, indent=1)
        f.write("\n")
    print(f"rowenc.json: {len(out)} cases")


if __name__ == "__main__":
    main()
