#!/usr/bin/env python3
"""Fixture of the snapshot-visible view, read as DATA from the
reference's testdata/iterator (run where the reference checkout is,
make_fixtures.REF; the tests read only the output):

  tests/golden/iterator_points.json
      every `iter seq=N` case of testdata/iterator whose `define` has no options
      and holds only `key#seq,KIND:value` lines of the six point kinds in sorted
      order, that has no option other than `seq`, and whose commands are all
      among first, last, next, prev, seek-ge K, seek-lt K: the define, the seq,
      the commands and the expected lines (without the `stats:` lines).  The
      cases left out need prefix seeks, limits, bounds or range keys.
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
COMMANDS = {"first": 0, "last": 0, "next": 0, "prev": 0, "seek-ge": 1, "seek-lt": 1}


def parse_define(text: str):
    """[(key, seq, kind, value)] in sorted order, or None when the define holds
    anything else."""
    kvs = []
    for line in text.split("\n"):
        if not line.strip():
            continue
        m = LINE.match(line.strip())
        if not m or m.group(3) not in KINDS:
            return None
        kvs.append((m.group(1), int(m.group(2)), m.group(3), m.group(4)))
    order = [(k.encode(), -s) for k, s, _, _ in kvs]
    return kvs if kvs and order == sorted(order) else None


def main():
    cases, define = [], None
    for c in parse_datadriven(os.path.join(REF, "testdata", "iterator")):
        words = c["cmd"].split()
        if words[0] == "define":
            define = parse_define(c["input"]) if len(words) == 1 else None
            continue
        if words[0] != "iter" or define is None or len(words) != 2 or not re.fullmatch(r"seq=\d+", words[1]):
            continue
        cmds = [ln.split() for ln in c["input"].split("\n") if ln.strip()]
        if not cmds or any(w[0] not in COMMANDS or len(w) != 1 + COMMANDS[w[0]] for w in cmds):
            continue
        expected = [ln for ln in c["expected"].split("\n") if ln.strip() and not ln.startswith("stats:")]
        cases.append({"define": [list(kv) for kv in define], "seq": int(words[1][4:]),
                      "commands": [" ".join(w) for w in cmds], "expected": expected})
    out = os.path.join(HERE, "iterator_points.json")
    with open(out, "w") as f:
        json.dump({"source": "testdata/iterator", "kinds": KINDS, "cases": cases}, f, indent=1)
        f.write("\n")
    print(out, len(cases), "cases,", sum(len(c["expected"]) for c in cases), "lines,",
          sum(1 for c in cases if any(kv[2] == "MERGE" for kv in c["define"])), "with MERGE")


if __name__ == "__main__":
    main()
