#!/usr/bin/env python3
"""Fixture of the compaction view, read as DATA from the
reference's internal/compact/testdata (run where the reference checkout is,
make_fixtures.REF; the tests read only the output):

  tests/golden/compact_iter.json
      every `iter` case of testdata/iter, iter_set_with_del and
      iter_delete_sized whose `define` has no options and holds only
      `key#seq,KIND:value` lines of the six point kinds in strictly sorted
      order (no spans, RANGEDEL, blobref( or INVALID), whose options are among
      snapshots, elide-tombstones, is-bottommost-layer, print-snapshot-pinned,
      print-missized-dels and print-missized-del-info, and whose expected text
      holds no `err=`.  `varint(N)` values are stored as the uvarint's bytes
      (hex, as every value), the debug merger's `[base]` marker is stripped
      from expected values, and the callback lines become expected counts.
      `complete` is false for the few cases whose commands stop at the last
      result, before the final `.`: their results are all there is to compare.
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
OUT_LINE = re.compile(r"^([^#\s]+)#(\d+),([A-Z]+):(.*?)( \((not )?pinned\))?$")
OPTIONS = {"snapshots", "elide-tombstones", "is-bottommost-layer", "print-snapshot-pinned", "print-missized-dels",
           "print-missized-del-info"}
TRUE = {"1", "t", "T", "TRUE", "true", "True"}  # strconv.ParseBool
FILES = ["iter", "iter_set_with_del", "iter_delete_sized"]


def uvarint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def value_bytes(text: str) -> bytes:
    m = re.fullmatch(r"varint\((\d+)\)", text)
    return uvarint(int(m.group(1))) if m else text.encode()


def parse_define(text: str):
    """[(key, seq, kind, value hex)] in strictly sorted order, or None when the
    define holds anything else."""
    kvs = []
    for line in text.split("\n"):
        if not line.strip():
            continue
        m = LINE.match(line.strip())
        if not m or m.group(3) not in KINDS or "blobref(" in line or "INVALID" in line:
            return None
        kvs.append((m.group(1), int(m.group(2)), m.group(3), value_bytes(m.group(4)).hex()))
    order = [(k.encode(), -s) for k, s, _, _ in kvs]
    strictly = all(a < b for a, b in zip(order, order[1:]))
    return kvs if kvs and strictly else None


def parse_options(words):
    """{snapshots, elide, bottommost, pinned}, or None for an option outside OPTIONS."""
    o = {"snapshots": [], "elide": False, "bottommost": False, "pinned": False}
    for w in words:
        key, _, val = w.partition("=")
        if key not in OPTIONS:
            return None
        if key == "snapshots":
            o["snapshots"] = sorted(int(v) for v in val.strip("()").split(",") if v)
        elif key == "elide-tombstones":
            o["elide"] = val in TRUE
        elif key == "is-bottommost-layer":
            o["bottommost"] = val in TRUE
        elif key == "print-snapshot-pinned":
            o["pinned"] = True
    return o


def main():
    cases = []
    for name in FILES:
        define = None
        for c in parse_datadriven(os.path.join(REF, "internal", "compact", "testdata", name)):
            words = c["cmd"].split()
            if words[0] == "define":
                define = parse_define(c["input"]) if len(words) == 1 else None
                continue
            if words[0] != "iter" or define is None:
                continue
            opt = parse_options(words[1:])
            if opt is None or "err=" in c["expected"]:
                continue
            cmds = [ln.strip() for ln in c["input"].split("\n") if ln.strip()]
            assert cmds[0] == "first" and all(x == "next" for x in cmds[1:]), (name, cmds)
            results, counts, missized_printed = [], {"missized": 0, "ineffectual": 0, "nondeterministic": 0}, False
            lines = [ln for ln in c["expected"].split("\n") if ln.strip()]
            done = False
            for ln in lines:
                if ln == ".":
                    done = True
                elif ln.startswith("missized-dels="):
                    counts["missized"] = int(ln.split("=")[1])
                    missized_printed = True
                elif ln.startswith("ineffectual-single-deletes:"):
                    counts["ineffectual"] = len(ln.split(":", 1)[1].strip().split(","))
                elif ln.startswith("invariant-violation-single-deletes:"):
                    counts["nondeterministic"] = len(ln.split(":", 1)[1].strip().split(","))
                elif ln.startswith("missized-delete-info:"):
                    if not missized_printed:
                        counts["missized"] = len(ln.split(":", 1)[1].strip().split(";"))
                        missized_printed = True
                else:
                    m = OUT_LINE.match(ln)
                    assert m and not done, (name, ln)
                    v = m.group(4)
                    if v.endswith("[base]"):
                        v = v[: -len("[base]")]
                    r = [m.group(1), int(m.group(2)), m.group(3), value_bytes(v).hex()]
                    if opt["pinned"]:
                        assert m.group(5), (name, ln)
                        r.append(0 if m.group(6) else 1)
                    results.append(r)
            cases.append({"file": name, "define": [list(kv) for kv in define], "snapshots": opt["snapshots"],
                          "elide": opt["elide"], "bottommost": opt["bottommost"], "print_pinned": opt["pinned"],
                          "missized_known": missized_printed, "complete": done, "results": results, **counts})
    out = os.path.join(HERE, "compact_iter.json")
    with open(out, "w") as f:
        json.dump({"source": "internal/compact/testdata/{iter,iter_set_with_del,iter_delete_sized}", "kinds": KINDS,
                   "cases": cases}, f, indent=1)
        f.write("\n")

    def has(c, kind):
        return any(kv[2] == kind for kv in c["define"])
    print(out, len(cases), "cases,", sum(len(c["results"]) for c in cases), "result lines,",
          sum(1 for c in cases if c["snapshots"]), "with snapshots,", sum(1 for c in cases if has(c, "SINGLEDEL")),
          "SINGLEDEL,", sum(1 for c in cases if has(c, "DELSIZED")), "DELSIZED,", sum(1 for c in cases if has(c, "MERGE")),
          "MERGE,", sum(1 for c in cases if c["elide"]), "with elision,", sum(1 for c in cases if c["print_pinned"]),
          "print pinned,", sum(1 for c in cases if not c["complete"]), "stop before the final '.',",
          sum(1 for c in cases if c["missized_known"] or c["ineffectual"] or c["nondeterministic"]), "with a callback or missized line")


if __name__ == "__main__":
    main()
