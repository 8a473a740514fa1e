#!/usr/bin/env python3
"""Fixture of the whole read path ("Tests"), read as DATA from
the reference's testdata/iter_histories/* and testdata/iterator (run where the
reference checkout is, make_fixtures.REF; the tests read only the output):

  tests/golden/iter_histories.json
      "sections": per `reset` of every file the writes that follow it, in order:
          {"ops": [[op, field, ...], ...]}    a `batch commit`
          {"populate": {keylen, timestamps, prefix}}
      "segments": the forward segments of the `combined-iter` scripts: the
          section, how many of its writes had happened, lower / upper /
          mask_suffix (null = unset), the start (null = `first`, else the
          `seek-ge` key) and the expected lines, parsed:
          null (exhausted) or [key, value or null, span or null],
          span = [start, end, [[suffix, value], ...]].
      "iterator": the `iter seq=N lower=.. upper=..` cases of testdata/iterator
          over an option-less, points-only `define` (the cases
          make_visible_fixtures.py leaves out for their bounds only), cut into
          forward segments by the same rule.
      "excluded": how many scripts and segments each rule below left out.

A *history* is the list of writes since the last `reset`.  Writes: `batch
commit` whose lines are all set / del / singledel / merge / del-range /
range-key-set / range-key-unset / range-key-del, and `populate` without
`vallen=`.  IGNORED commands do not change what an iterator returns.  Anything
else TAINTS the history until the next `reset`: any other command, a batch that
is not `batch commit`, a `reset` option outside RESET_OPTIONS.  A
`combined-iter` script is taken when the history is untainted and every option
is among ITER_OPTIONS.  It is cut at its first set-options / set-bounds / clone;
the rest is cut into forward segments: a `first` or `seek-ge K` and the plain
`next` lines after it.  Any other command ends the segment and is skipped with
its output line.  Commands and expected lines correspond one to one: a script
where they do not is dropped, and so is a segment with a line that is neither
`.` nor `key: (value-or-., span-or-.)`.  The UPDATED token is dropped
(RangeKeyChanged is not part of read()'s contract).  Strings are stored as
latin-1 text of the bytes (the reference's %q quoting undone).
"""
from __future__ import annotations

import ast
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF, parse_datadriven  # noqa: E402
from make_visible_fixtures import KINDS, parse_define  # noqa: E402

WRITE_OPS = {"set": 3, "del": 2, "singledel": 2, "merge": 3, "del-range": 3, "range-key-set": (4, 5),
             "range-key-unset": 4, "range-key-del": 3}
IGNORED = {"flush", "compact", "lsm", "metrics", "iter", "clone", "get", "rangekey-iter", "scan-rangekeys", "layout",
           "wait-table-stats"}
RESET_OPTIONS = {"block-size", "index-block-size", "bloom-bits-per-key", "target-file-sizes", "format-major-version"}
ITER_OPTIONS = {"lower", "upper", "mask-suffix", "mask-filter", "key-types"}
CUTS = {"set-options", "set-bounds", "clone"}

QUOTED = r'"(?:[^"\\]|\\.)*"'
KEY = r"(?:%s|[A-Za-z\[\]\\^_`]+)" % QUOTED
LINE = re.compile(r"^(\S+): \((.*)\)$")
SPAN = re.compile(r"^\[(%s)-(%s)\)(.*)$" % (KEY, KEY))


def options(cmd: str):
    """'combined-iter lower=b timestamps=(1, 10)' -> {'lower': 'b', 'timestamps': '1, 10'}; a bare word maps to None."""
    out = {}
    for m in re.finditer(r"([\w-]+)(?:=(\([^)]*\)|\S*))?", cmd.split(None, 1)[1] if " " in cmd.strip() else ""):
        v = m.group(2)
        out[m.group(1)] = v[1:-1] if v is not None and v.startswith("(") else v
    return out


def unquote(s: str):
    if not s.startswith('"'):
        return s
    return ast.literal_eval("b" + s).decode("latin-1")


def parse_batch(text: str):
    """[[op, field, ...]] as runBatchDefineCmd splits them, or None for a line outside WRITE_OPS."""
    ops = []
    for line in text.split("\n"):
        f = line.split()
        if not f:
            continue
        n = WRITE_OPS.get(f[0])
        if n is None:
            return None
        lo, hi = n if isinstance(n, tuple) else (n, n)
        if len(f) < lo:
            return None
        if len(f) > hi:
            f = f[: hi - 1] + [" ".join(f[hi - 1:])]
        if any(x.startswith("<") for x in f):  # (<nil>, <rand-bytes=N>)
            return None
        ops.append(f)
    return ops


def parse_line(line: str):
    """null for '.', [key, value, span] for a position, or an Exception for anything else."""
    if line == ".":
        return None
    m = LINE.match(line)
    if not m:
        raise ValueError(line)
    inner = m.group(2)
    if inner.endswith(" UPDATED"):
        inner = inner[: -len(" UPDATED")]
    q = re.match(QUOTED, inner)
    cut = q.end() if q else inner.index(", ")
    if inner[cut: cut + 2] != ", ":
        raise ValueError(line)
    value, rest = inner[:cut], inner[cut + 2:]
    span = None
    if rest != ".":
        s = SPAN.match(rest)
        if not s:
            raise ValueError(line)
        keys = []
        for part in s.group(3).split(","):
            part = part.strip()
            if not part:
                continue
            sfx, _, val = part.partition("=")
            keys.append([sfx, unquote(val)])
        span = [unquote(s.group(1)), unquote(s.group(2)), keys]
    return [m.group(1), None if value == "." else unquote(value), span]


def forward_segments(cmds, expected, count):
    """[(start, lines)]: `first` / `seek-ge K` and the plain `next` lines after it."""
    segs, cur = [], None
    for w, line in zip(cmds, expected):
        if w == ["first"] or (w[0] == "seek-ge" and len(w) == 2):
            cur = [w[1] if len(w) == 2 else None, [line]]
            segs.append(cur)
        elif w == ["next"] and cur is not None:
            cur[1].append(line)
        else:
            cur = None
    out = []
    for start, lines in segs:
        try:
            out.append((start, [parse_line(ln) for ln in lines]))
        except (ValueError, SyntaxError):
            count["segments_with_an_unparsed_line"] += 1
    return out


def cut_script(text: str):
    cmds = [ln.split() for ln in text.split("\n") if ln.strip()]
    for i, w in enumerate(cmds):
        if w[0] in CUTS:
            return cmds, cmds[:i]
    return cmds, cmds


def histories(count):
    sections, segments = [], []
    d = os.path.join(REF, "testdata", "iter_histories")
    for name in sorted(os.listdir(d)):
        tainted, section = True, None  # (no database before the first reset)
        for c in parse_datadriven(os.path.join(d, name)):
            word = c["cmd"].split()[0]
            if word == "reset":
                tainted = bool(set(options(c["cmd"])) - RESET_OPTIONS)
                section = {"file": name, "writes": []}
                sections.append(section)
            elif word in IGNORED:
                pass
            elif word == "batch":
                ops = parse_batch(c["input"]) if c["cmd"].split() == ["batch", "commit"] else None
                if ops is None or tainted:
                    tainted = True
                else:
                    section["writes"].append({"ops": ops})
            elif word == "populate":
                o = options(c["cmd"])
                if set(o) - {"keylen", "timestamps", "prefix"} or tainted:
                    tainted = True
                else:
                    ts = [int(x) for x in (o.get("timestamps") or "1").replace(",", " ").split()]
                    section["writes"].append({"populate": {"keylen": int(o["keylen"]), "timestamps": ts,
                                                           "prefix": o.get("prefix") or ""}})
            elif word == "combined-iter":
                count["scripts"] += 1
                o = options(c["cmd"])
                if tainted:
                    count["scripts_on_a_tainted_history"] += 1
                    continue
                if set(o) - ITER_OPTIONS or o.get("key-types", "both") != "both":
                    count["scripts_with_another_option"] += 1
                    continue
                cmds, kept = cut_script(c["input"])
                expected = [ln for ln in c["expected"].split("\n") if ln.strip()]
                if len(cmds) != len(expected):
                    count["scripts_whose_lines_do_not_correspond"] += 1
                    continue
                segs = forward_segments(kept, expected, count)
                if not segs:
                    count["scripts_without_a_forward_segment"] += 1
                    continue
                count["scripts_taken"] += 1
                for start, lines in segs:
                    segments.append({"section": sections.index(section), "n_writes": len(section["writes"]),
                                     "lower": o.get("lower"), "upper": o.get("upper"), "mask_suffix": o.get("mask-suffix"),
                                     "start": start, "lines": lines})
            else:
                tainted = True
    used = sorted({s["section"] for s in segments})
    for s in segments:
        s["section"] = used.index(s["section"])
    return [sections[i] for i in used], segments


def iterator_cases(count):
    cases, define = [], None
    for c in parse_datadriven(os.path.join(REF, "testdata", "iterator")):
        words = c["cmd"].split()
        if words[0] == "define":
            define = parse_define(c["input"]) if len(words) == 1 else None
            continue
        o = options(c["cmd"]) if words[0] == "iter" else {}
        if words[0] != "iter" or define is None or not (set(o) & {"lower", "upper"}):
            continue
        count["iterator_scripts"] += 1
        if set(o) - {"seq", "lower", "upper"} or not re.fullmatch(r"\d+", o.get("seq") or ""):
            count["iterator_scripts_with_another_option"] += 1
            continue
        cmds, kept = cut_script(c["input"])
        expected = [ln for ln in c["expected"].split("\n") if ln.strip() and not ln.startswith("stats:")]
        if len(cmds) != len(expected):
            count["iterator_scripts_whose_lines_do_not_correspond"] += 1
            continue
        for start, lines in forward_segments(kept, expected, count):
            cases.append({"define": [list(kv) for kv in define], "seq": int(o["seq"]), "lower": o.get("lower"),
                          "upper": o.get("upper"), "start": start, "lines": lines})
    return cases


def main():
    count = {k: 0 for k in ("scripts", "scripts_taken", "scripts_on_a_tainted_history", "scripts_with_another_option",
                            "scripts_whose_lines_do_not_correspond", "scripts_without_a_forward_segment",
                            "segments_with_an_unparsed_line", "iterator_scripts", "iterator_scripts_with_another_option",
                            "iterator_scripts_whose_lines_do_not_correspond")}
    sections, segments = histories(count)
    cases = iterator_cases(count)
    out = os.path.join(HERE, "iter_histories.json")
    with open(out, "w") as f:
        json.dump({"source": "testdata/iter_histories, testdata/iterator", "excluded": count, "kinds": KINDS,
                   "sections": sections, "segments": segments, "iterator": cases}, f, separators=(",", ":"))
        f.write("\n")

    def has(seg, *ops):
        return any(op[0] in ops for w in sections[seg["section"]]["writes"][: seg["n_writes"]] for op in w.get("ops", []))

    print(out, count)
    print(len(segments), "segments,", sum(len(s["lines"]) for s in segments), "lines,",
          sum(1 for s in segments if has(s, "range-key-set", "range-key-unset", "range-key-del")), "over range keys,",
          sum(1 for s in segments if s["mask_suffix"] is not None), "with a mask suffix,",
          sum(1 for s in segments if has(s, "del-range")), "over a del-range,",
          sum(1 for s in segments for ln in s["lines"] if ln and ln[2]), "lines with a span;",
          len(cases), "iterator segments,", sum(len(c["lines"]) for c in cases), "lines")


if __name__ == "__main__":
    main()
