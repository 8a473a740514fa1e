#!/usr/bin/env python3
"""Fixture of the range deletions in the read path, read as
DATA from the reference's test data (run where the reference checkout is,
make_fixtures.REF; the tests read only the output):

  tests/golden/range_del.json
      defines   every option-less `define` of testdata/range_del that is
                followed by `get seq=N` / `iter seq=N` cases: its sections
                (`mem`, `L0`..`L3`) with their `key#seq,KIND:value` lines in
                listed order, and those cases (an `iter` only when its
                commands are all among first, last, next, prev, seek-ge K,
                seek-lt K): the sequence number, the input lines and the
                expected lines.
                Left out: the defines with `target-file-sizes` (compactions
                move their contents) and a define in which a section at a
                shallower level (mem above L0 above L1 ...) holds a sequence
                number smaller than one in a deeper level.  Only there do the
                reference's level-by-level rule and the pure sequence-number
                rule disagree; sections of the same level are unconstrained.
                That rule drops exactly the define under the reference's
                comment "Invalid LSM structure" (asserted below).
      fragments the `build` inputs of sstable/rowblk/testdata/rowblk_fragment_iter
                and their fragmented outputs: they pin the Python fragmenter of
                tests/rangedelutil.py.
"""
from __future__ import annotations

import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF, parse_datadriven  # noqa: E402

KINDS = {"DEL": 0, "SET": 1, "MERGE": 2, "SINGLEDEL": 7, "RANGEDEL": 15, "SETWITHDEL": 18, "RANGEKEYDEL": 19,
         "RANGEKEYUNSET": 20, "RANGEKEYSET": 21, "DELSIZED": 23}
LINE = re.compile(r"^([^#\s]+)#(\d+),([A-Z]+):(.*)$")
SECTION = re.compile(r"^(mem|L\d+)$")
SPAN = re.compile(r"^(\S+?)-(\S+?):\{(.*)\}$")
COMMANDS = {"first": 0, "last": 0, "next": 0, "prev": 0, "seek-ge": 1, "seek-lt": 1}


def level(name: str) -> int:
    return -1 if name == "mem" else int(name[1:])


def parse_define(text: str):
    """[{"level": name, "kvs": [[key, seq, kind, value]]}] in listed order."""
    sections = []
    for line in text.split("\n"):
        if not line.strip():
            continue
        if SECTION.match(line):
            sections.append({"level": line, "kvs": []})
            continue
        m = LINE.match(line.strip())
        assert m and line.startswith(" ") and sections and m.group(3) in KINDS, line
        sections[-1]["kvs"].append([m.group(1), int(m.group(2)), m.group(3), m.group(4)])
    return sections


def lsm_ordered(sections) -> bool:
    """No shallower section holds a sequence number smaller than one in a deeper level."""
    for a in sections:
        for b in sections:
            if level(a["level"]) < level(b["level"]) and a["kvs"] and b["kvs"]:
                if min(kv[1] for kv in a["kvs"]) < max(kv[1] for kv in b["kvs"]):
                    return False
    return True


def parse_spans(text: str):
    out = []
    for line in text.split("\n"):
        if not line.strip():
            continue
        m = SPAN.match(line.strip())
        assert m, line
        out.append({"start": m.group(1), "end": m.group(2), "keys": re.findall(r"\(([^)]*)\)", m.group(3))})
    return out


def main():
    path = os.path.join(REF, "testdata", "range_del")
    raw = open(path).read().split("\n")
    at = next(i for i, ln in enumerate(raw) if ln.startswith("# Invalid LSM structure"))
    d0 = next(i for i in range(at, len(raw)) if raw[i] == "define")
    invalid_text = "\n".join(raw[d0 + 1: raw.index("----", d0)])

    defines, cur, state = [], None, None
    dropped, with_options, before_options = [], 0, 0
    for c in parse_datadriven(path):
        words = c["cmd"].split()
        if words[0] == "define":
            cur = None
            if len(words) > 1:
                assert words[1].startswith("target-file-sizes"), c["cmd"]
                with_options += 1
                state = "options"
                continue
            sections = parse_define(c["input"])
            if not lsm_ordered(sections):
                dropped.append(c["input"])
                state = "dropped"
                continue
            state = "kept"
            cur = {"sections": sections, "cases": []}
            defines.append(cur)
            if not with_options:
                before_options += 1
            continue
        if cur is None or words[0] not in ("get", "iter"):
            continue
        assert len(words) == 2 and re.fullmatch(r"seq=\d+", words[1]), c["cmd"]
        inp = [ln.strip() for ln in c["input"].split("\n") if ln.strip()]
        if words[0] == "iter":
            cmds = [ln.split() for ln in inp]
            if any(w[0] not in COMMANDS or len(w) != 1 + COMMANDS[w[0]] for w in cmds):
                continue
        exp = [ln for ln in c["expected"].split("\n") if ln.strip()]
        assert len(exp) == len(inp), c
        cur["cases"].append({"op": words[0], "seq": int(words[1][4:]), "input": inp, "expected": exp})
    # the conditions the selection rests on
    assert dropped == [invalid_text], dropped
    assert with_options == 4, with_options
    assert before_options == 7, before_options  # every option-less define before them but the invalid one
    after = [d for d in defines[before_options:]]
    defines = [d for d in defines if d["cases"]]
    assert len(defines) == before_options + sum(1 for d in after if d["cases"]) and len(defines) > before_options
    assert all(any(kv[2] == "RANGEDEL" for s in d["sections"] for kv in s["kvs"]) or len(d["sections"]) > 1
               for d in defines)
    n_cases = sum(len(d["cases"]) for d in defines)
    n_lines = sum(len(c["expected"]) for d in defines for c in d["cases"])

    frags = []
    for c in parse_datadriven(os.path.join(REF, "sstable", "rowblk", "testdata", "rowblk_fragment_iter")):
        if c["cmd"].split()[0] == "build":
            frags.append({"input": parse_spans(c["input"]), "output": parse_spans(c["expected"])})
    assert len(frags) == 3

    out = os.path.join(HERE, "range_del.json")
    with open(out, "w") as f:
        json.dump({"source": ["testdata/range_del", "sstable/rowblk/testdata/rowblk_fragment_iter"], "kinds": KINDS,
                   "n_defines": len(defines), "n_cases": n_cases, "n_lines": n_lines, "defines": defines,
                   "fragments": frags}, f, indent=1)
        f.write("\n")
    print(out, len(defines), "defines,", n_cases, "cases,", n_lines, "lines,", len(frags), "fragment builds")


if __name__ == "__main__":
    main()
