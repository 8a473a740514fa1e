"""Helpers of the range-key tests (tests/test_rangekey.py, tests/test_rangekey_gpu.py).

A third statement of include/pebble_amd.h's range-key rules, written from the
prose and sharing nothing with the library but the user-key order
(pebble_amd.blockiter.key_compare, as rangedelutil does): `suffix_cmp`
(CompareRangeSuffixes), `coalesce`, `expected_spans` (merge, coalesce,
defragment), `clip_spans`, `expected_masked`.  It is pinned by the reference's
own data files, transcribed in tests/golden/rangekey.json.  `layout` lays spans
out as `Decoded.to_host()` does, so that host and device results are compared
byte for byte; `run_host` makes a run of fragmented spans through
keyspanutil's Python block decoder.  `with_range_keys` re-emits a golden
columnar table with a `pebble.range_key` keyspan block."""
import functools
import json
import os
import re

import numpy as np

from keyspanutil import block_of_spans, expected as decode_blocks
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare

D, T, C = N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB
DEL, UNSET, SET = 19, 20, 21
KINDS = {"RANGEKEYDEL": DEL, "RANGEKEYUNSET": UNSET, "RANGEKEYSET": SET}
MAX = N.PBL_SEQNUM_MAX
ALL = N.PBL_RANGEDEL_ALL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangekey.json")
SYN = b"_synthetic"


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def tr(seq, kind=SET):
    return seq << 8 | kind


# ---- CompareRangeSuffixes, Split --------------------------------------------------------------------
def _sign(x):
    return (x > 0) - (x < 0)


def _bcmp(a, b):
    return _sign((a > b) - (a < b))


def suffix_cmp(comparer, a: bytes, b: bytes) -> int:
    if comparer == T:
        # compareSuffixes: the timestamps, newer first, the empty suffix first of all; of two equal ones
        # the one without the "_synthetic" mark first
        at = a[:-len(SYN)] if a.endswith(SYN) else a
        bt = b[:-len(SYN)] if b.endswith(SYN) else b
        if not at or not bt:
            c = _bcmp(len(at), len(bt))
        else:
            c = _bcmp(int(bt[1:]), int(at[1:]))
        if c == 0 and (at != a) != (bt != b):
            c = 1 if at != a else -1
        return c
    if comparer == C:
        if not a or not b:
            return _bcmp(len(a), len(b))
        return _bcmp(b[:-1], a[:-1])
    return _bcmp(a, b)


def split(comparer, key: bytes) -> int:
    if comparer == T:
        i = key.rfind(b"@")
        return i if i >= 0 else len(key)
    if comparer == C:
        if not key:
            return 0
        return len(key) - key[-1] if key[-1] <= len(key) else 0
    return len(key)


# ---- the reference's notation -------------------------------------------------------------------------
def parse_span(line: str):
    """'a-c:{(#10,RANGEKEYSET,@5,foo) (#10,RANGEKEYDEL)}' -> (b'a', b'c', [(trailer, suffix, value)])."""
    m = re.fullmatch(r"(\w+)-(\w+):\{(.*)\}", line.strip())
    keys = []
    for k in re.findall(r"\(([^)]*)\)", m.group(3)):
        f = k.split(",")
        keys.append((tr(int(f[0][1:]), KINDS[f[1]]), (f[2] if len(f) > 2 else "").encode(),
                     (f[3] if len(f) > 3 else "").encode()))
    return m.group(1).encode(), m.group(2).encode(), keys


def sets_of(keys, comparer=T):
    """The internal-keys form of an expected span reduced to the user form: the sets, in suffix order."""
    s = [k for k in keys if k[0] & 0xff == SET]
    return sorted(s, key=functools.cmp_to_key(lambda a, b: suffix_cmp(comparer, a[1], b[1])))


# ---- the rules ------------------------------------------------------------------------------------------
def visible(seq, snapshot):
    return snapshot >= MAX or seq < snapshot


def coalesce(keys, comparer, snapshot=MAX):
    """keys: [(trailer, suffix, value)] in (trailer descending, run, index) order
    -> the surviving sets [(trailer, suffix, value)] by suffix ascending."""
    vis = [k for k in keys if visible(k[0] >> 8, snapshot)]
    cut = max((k[0] for k in vis if k[0] & 0xff == DEL), default=-1)
    count = [k for k in vis if k[0] > cut]
    winners = []
    for k in count:  # the first key of every group of compare-equal suffixes
        if not any(suffix_cmp(comparer, w[1], k[1]) == 0 for w in winners):
            winners.append(k)
    sets = [w for w in winners if w[0] & 0xff == SET]
    return sorted(sets, key=functools.cmp_to_key(lambda a, b: suffix_cmp(comparer, a[1], b[1])))


def _covering(runs, comparer, lo, hi):
    """Every key of every fragment with start <= lo and hi <= end, by (trailer descending, run, index)."""
    keys = []
    for r, spans in enumerate(runs):
        i = 0
        for s, e, ks in spans:
            for k in ks:
                if key_compare(comparer, s, lo) <= 0 and key_compare(comparer, hi, e) <= 0:
                    keys.append((k, r, i))
                i += 1
    keys.sort(key=lambda x: (-x[0][0], x[1], x[2]))
    return [k for k, _, _ in keys]


def expected_spans(runs, comparer, snapshot=MAX, defrag=True):
    """runs: per run its fragmented spans [(start, end, [(trailer, suffix, value)])]
    -> the coalesced, defragmented spans in the same form (sets in suffix order)."""
    bs = [b for spans in runs for s, e, _ in spans for b in (s, e)]
    bs.sort(key=functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b)))  # (stable)
    uniq = []
    for b in bs:
        if not uniq or key_compare(comparer, uniq[-1], b) != 0:
            uniq.append(b)
    out, open_ = [], False
    for lo, hi in zip(uniq, uniq[1:]):
        sets = coalesce(_covering(runs, comparer, lo, hi), comparer, snapshot)
        if not sets:
            open_ = False
            continue
        prev = out[-1][2] if open_ else None
        if defrag and prev is not None and len(prev) == len(sets) and all(
                suffix_cmp(comparer, a[1], b[1]) == 0 and a[2] == b[2] for a, b in zip(prev, sets)):
            out[-1] = (out[-1][0], hi, prev)
        else:
            out.append((lo, hi, sets))
        open_ = True
    return out


def clip_spans(spans, lower, upper, comparer):
    """The spans that intersect [lower, upper) (None = unbounded), truncated to it."""
    out = []
    for s, e, ks in spans:
        if lower is not None and key_compare(comparer, e, lower) <= 0:
            continue
        if upper is not None and key_compare(comparer, s, upper) >= 0:
            continue
        if lower is not None and key_compare(comparer, s, lower) < 0:
            s = lower
        if upper is not None and key_compare(comparer, upper, e) < 0:
            e = upper
        if key_compare(comparer, s, e) >= 0:  # (an empty or inverted range intersects nothing)
            continue
        out.append((s, e, ks))
    return out


def expected_masked(runs, key: bytes, comparer, t: bytes, snapshot=MAX) -> bool:
    """Whether the point `key` is masked under the runs at threshold suffix t."""
    p = key[split(comparer, key):]
    if not p:
        return False
    keys = []
    for r, spans in enumerate(runs):
        i = 0
        for s, e, ks in spans:
            for k in ks:
                if key_compare(comparer, s, key) <= 0 and key_compare(comparer, key, e) < 0:
                    keys.append((k, r, i))
                i += 1
    keys.sort(key=lambda x: (-x[0][0], x[1], x[2]))
    cand = [k[1] for k in coalesce([k for k, _, _ in keys], comparer, snapshot)
            if k[1] and suffix_cmp(comparer, k[1], t) >= 0]
    if not cand:
        return False
    r = min(cand, key=functools.cmp_to_key(lambda a, b: suffix_cmp(comparer, a, b)))
    return suffix_cmp(comparer, r, p) < 0


def expected_cover(runs, keys, comparer, t, snapshot=MAX, cover=None):
    out = [0] * len(keys) if cover is None else [int(c) for c in cover]
    for i, k in enumerate(keys):
        if expected_masked(runs, k, comparer, t, snapshot):
            out[i] = ALL
    return out


# ---- layouts ----------------------------------------------------------------------------------------------
def layout(blocks, statuses=None) -> dict:
    """blocks: per block its spans -> the set's form in `Decoded.to_host()`'s
    layout: one KV per (span, key), entry_off = the span's ordinal in its block,
    span = the index in the block of the span's first KV."""
    nb = len(blocks)
    statuses = list(statuses) if statuses is not None else [0] * nb
    t, eo, sp = [], [], []
    offs = {k: [] for k in "kvsx"}
    data = {k: bytearray() for k in "kvsx"}
    bases = {k: [0] for k in "nkvsx"}
    for spans in blocks:
        base = {k: len(data[k]) for k in "kvsx"}
        first = 0
        for o, (s, e, ks) in enumerate(spans):
            for trl, suffix, value in ks:
                for k, x in zip("kvsx", (s, e, suffix, value)):
                    offs[k].append(len(data[k]) - base[k])
                    data[k] += x
                t.append(trl)
                eo.append(o)
                sp.append(first)
            first += len(ks)
        for k in "kvsx":
            offs[k].append(len(data[k]) - base[k])
            bases[k].append(len(data[k]))
        bases["n"].append(len(t))
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy()  # noqa: E731
    mask = 0
    for s in statuses:
        mask |= (1 << s) if s else 0
    return {"trailer": np.array(t, np.uint64), "kv_flags": np.zeros(len(t), np.uint8), "entry_off": np.array(eo, np.uint32),
            "key_off": np.array(offs["k"], np.uint32), "val_off": np.array(offs["v"], np.uint32),
            "key_bytes": u8(data["k"]), "val_bytes": u8(data["v"]), "restarts": None,
            "blk_kv_base": np.array(bases["n"], np.uint64), "blk_key_base": np.array(bases["k"], np.uint64),
            "blk_val_base": np.array(bases["v"], np.uint64), "blk_rst_base": np.zeros(nb + 1, np.uint64),
            "blk_status": np.array(statuses, np.uint32), "n_kv": len(t), "key_bytes_total": len(data["k"]),
            "val_bytes_total": len(data["v"]), "n_restarts": 0, "status_mask": mask,
            "n_bad_blocks": sum(1 for s in statuses if s), "n_slow_blocks": 0,
            "span": np.array(sp, np.uint32), "suffix_off": np.array(offs["s"], np.uint32),
            "value_off": np.array(offs["x"], np.uint32), "suffix_bytes": u8(data["s"]), "value_bytes": u8(data["x"]),
            "blk_suffix_base": np.array(bases["s"], np.uint64), "blk_value_base": np.array(bases["x"], np.uint64)}


def empty_set(status) -> dict:
    return layout([[]], [status])


def run_block(spans) -> bytes:
    return block_of_spans(spans)


def run_host(spans) -> dict:
    """A run as `Decoded.to_host()` lays it out, from the spans' keyspan block
    through keyspanutil's Python decoder."""
    return decode_blocks([run_block(spans)])


def spans_of_host(h: dict, b: int = 0):
    """Block b of a set / run in to_host()'s layout back as spans."""
    kv0, kv1 = int(h["blk_kv_base"][b]), int(h["blk_kv_base"][b + 1])
    get = lambda off, data, base, j: bytes(data[int(base[b]) + int(off[kv0 + b + j]): int(base[b]) + int(off[kv0 + b + j + 1])])  # noqa: E731
    out = []
    for j in range(kv1 - kv0):
        s = get(h["key_off"], h["key_bytes"], h["blk_key_base"], j)
        e = get(h["val_off"], h["val_bytes"], h["blk_val_base"], j)
        k = (int(h["trailer"][kv0 + j]), get(h["suffix_off"], h["suffix_bytes"], h["blk_suffix_base"], j),
             get(h["value_off"], h["value_bytes"], h["blk_value_base"], j))
        if out and int(h["span"][kv0 + j]) != j:
            out[-1][2].append(k)
        else:
            out.append((s, e, [k]))
    return out


# ---- generated runs ---------------------------------------------------------------------------------------
def gen_key(i: int) -> bytes:
    return b"k%06d" % i


def random_runs(rng, n_runs, n_bounds, comparer=T, suffixes=4, seq_hi=1000, max_keys=3, values=2):
    """n_runs runs over n_bounds boundary keys dealt at random: fragmented spans
    with gaps, empty fragments and 1..max_keys keys each, suffixes and values
    from small pools so that keys shadow one another and neighbours join."""
    def sfx(i):
        if i == 0:
            return b""
        if comparer == T:
            return b"@%d" % i
        if comparer == C:
            return (i * 1000).to_bytes(8, "big") + b"\x09"
        return b"s%d" % i
    gk = (lambda i: gen_key(i) + b"\x00") if comparer == C else gen_key  # (a crdb key ends in its version's length)
    runs = []
    for _ in range(n_runs):
        picks = sorted(rng.sample(range(n_bounds), max(2, n_bounds // n_runs)))
        spans, j = [], 0
        while j + 1 < len(picks):
            lo, hi = gk(picks[j]), gk(picks[j + 1])
            if rng.random() < 0.05:
                hi = lo  # an empty fragment
            ks = []
            for _ in range(rng.randrange(1, max_keys + 1)):
                kind = rng.choice((SET, SET, SET, UNSET, DEL))
                ks.append((tr(rng.randrange(1, seq_hi), kind), b"" if kind == DEL else sfx(rng.randrange(suffixes)),
                           b"v%d" % rng.randrange(values) if kind == SET else b""))
            ks.sort(key=lambda k: -k[0])
            spans.append((lo, hi, ks))
            j += 2 if (hi == lo or rng.random() < 0.2) else 1  # an empty fragment is followed by a gap
        runs.append(spans)
    return runs


def chain(n, value_of=lambda i: b"v", suffix_of=lambda i: b"@5", keys=1, first=0):
    """n abutting fragments [k_i, k_i+1), each with `keys` sets."""
    return [(gen_key(first + i), gen_key(first + i + 1),
             [(tr(100 - j, SET), suffix_of(i) if j == 0 else b"@%d" % (50 + j), value_of(i)) for j in range(keys)])
            for i in range(n)]


def wide_interval(m, comparer=T):
    """One interval [a, z) with m candidate keys over 4 runs: repeated suffixes
    (every suffix about 3 times), UNSETs, one DEL low down, invisible keys on top."""
    def sfx(i):
        if comparer == T:
            return b"@%d" % i
        if comparer == C:
            return (i * 7).to_bytes(8, "big") + b"\x09"
        return b"s%04d" % i
    runs = [[] for _ in range(4)]
    keys = [[] for _ in range(4)]
    for c in range(m):
        seq = 10 + (c * 7919) % (3 * m)
        kind = DEL if c == m // 2 else (UNSET if c % 5 == 0 else SET)
        if kind == DEL:
            seq = 12
        keys[c % 4].append((tr(seq, kind), b"" if kind == DEL else sfx(c % max(m // 3, 1)),
                            b"val%d" % c if kind == SET else b""))
    for r in range(4):
        keys[r].sort(key=lambda k: -k[0])
        z = b"\x00" if comparer == C else b""
        runs[r] = [(b"a" + z, b"z" + z, keys[r])] if keys[r] else []
    return runs


def cases():
    """(name, runs, comparer, snapshots): the shapes the issue lists that need no device."""
    import random
    out = []
    S = lambda seq, sfx, v: (tr(seq, SET), sfx, v)  # noqa: E731
    U = lambda seq, sfx: (tr(seq, UNSET), sfx, b"")  # noqa: E731
    X = lambda seq: (tr(seq, DEL), b"", b"")  # noqa: E731
    out.append(("no runs", [], T, (MAX,)))
    out.append(("an empty run", [[]], T, (MAX,)))
    out.append(("one set", [[(b"a", b"b", [S(5, b"@3", b"v")])]], T, (MAX, 5, 6)))
    out.append(("only unset and del", [[(b"a", b"b", [U(7, b"@3"), X(5)]), (b"b", b"c", [X(9)])]], T, (MAX,)))
    out.append(("set over unset at one seq", [[(b"a", b"b", [S(5, b"@3", b"v"), U(5, b"@3")])]], T, (MAX,)))
    out.append(("unset over set across runs at one seq", [[(b"a", b"b", [U(5, b"@3")])], [(b"a", b"b", [S(5, b"@3", b"v")])]],
                T, (MAX,)))
    out.append(("del spares its own seq", [[(b"a", b"c", [S(10, b"@5", b"x"), U(10, b"@4"), X(10), S(9, b"@4", b"y"),
                                                         S(4, b"@3", b"z")])]], T, (MAX, 10, 11)))
    out.append(("del at or above the snapshot", [[(b"a", b"c", [X(12), X(10), S(9, b"@4", b"y"), S(4, b"@3", b"z")])]], T,
                (10, 11, 12, 13)))
    out.append(("keys at the snapshot", [[(b"a", b"c", [S(9, b"@4", b"y"), S(8, b"@4", b"old"), U(8, b"@3"),
                                                        S(4, b"@3", b"z")])]], T, (8, 9, 10)))
    for m in (65, 257):
        out.append(("%d candidates" % m, wide_interval(m), T, (MAX, 10 + m)))
    out.append(("65 candidates crdb", wide_interval(65, C), C, (MAX,)))
    out.append(("65 candidates default", wide_interval(65, D), D, (MAX,)))
    for n_runs in (2, 16):
        out.append(("600 boundaries over %d runs" % n_runs, random_runs(random.Random(n_runs), n_runs, 600), T, (MAX, 500)))
    out.append(("chain of 300", [chain(300)], T, (MAX,)))
    out.append(("chain of 300 over 2 runs", [chain(300)[0::2], chain(300)[1::2]], T, (MAX,)))
    out.append(("chain with one other value", [chain(300, lambda i: b"w" if i == 150 else b"v")], T, (MAX,)))
    out.append(("chain with one other value byte in 3 keys", [chain(300, lambda i: b"vw" if i == 150 else b"vv", keys=3)], T,
                (MAX,)))
    broken = chain(40)
    broken[20] = (broken[20][0], broken[20][1], [U(200, b"@5")] + broken[20][2])
    out.append(("chain broken by an empty interval", [broken], T, (MAX, 150)))
    out.append(("chain broken by a gap", [chain(10) + chain(10, first=11)], T, (MAX,)))
    # suffixes that compare equal and differ in bytes: testkeys parses the number, so @07 is @7; crdb
    # leaves out the length byte.  (A "_synthetic" mark and a crdb synthetic bit do NOT compare equal
    # under CompareRangeSuffixes, whatever the point comparers do: the reference's coalesce data pins that.)
    out.append(("equal suffixes, other bytes", [chain(6, suffix_of=lambda i: b"@07" if i % 2 else b"@7")], T, (MAX,)))
    out.append(("synthetic mark is another suffix", [chain(6, suffix_of=lambda i: b"@7_synthetic" if i % 2 else b"@7"),
                                                     [(gen_key(0), gen_key(6), [S(300, b"@7_synthetic", b"s")])]], T,
                (MAX, 200)))
    w = (5).to_bytes(8, "big")
    ck = lambda i: b"k%02d\x00" % i  # noqa: E731
    out.append(("crdb equal suffixes, other bytes",
                [[(ck(i), ck(i + 1), [S(9, w + (b"\x09" if i % 2 else b"\x0a"), b"v")]) for i in range(6)]], C, (MAX,)))
    out.append(("crdb synthetic bit is another suffix",
                [[(ck(i), ck(i + 1), [S(9, w + (bytes(4) + b"\x01\x0e" if i % 2 else bytes(4) + b"\x0d"), b"v")])
                  for i in range(6)]], C, (MAX,)))
    for cmpr in (D, T, C):
        out.append(("random %d" % cmpr, random_runs(random.Random(70 + cmpr), 5, 120, cmpr), cmpr, (MAX, 400)))
    return out


def points_for(runs, comparer, extra=()):
    """Point user keys around every boundary of the runs: the boundary itself
    (no suffix) and the boundary with a few suffixes; sorted under the comparer."""
    bs = []
    for spans in runs:
        for s, e, _ in spans:
            bs += [s, e]
    pts = set(extra)
    for b in set(bs):
        pts.add(b)
        if comparer == T:
            pts.update(b + b"@%d" % n for n in (0, 2, 6, 40, 500))
        elif comparer == C and b.endswith(b"\x00"):
            pts.update(b + n.to_bytes(8, "big") + b"\x09" for n in (1, 4, 6, 21, 3000))
    return sorted(pts, key=functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b)))


# ---- a golden columnar table with range keys -------------------------------------------------------------
def with_range_keys(data: bytes, spans, block: bytes = None) -> bytes:
    """keyspanutil.with_range_dels for the metaindex's `pebble.range_key` entry
    (sstable/table.go:229): `data`, a columnar table, re-emitted with an appended
    keyspan block of `spans`, a new metaindex and a new footer."""
    import keyspanutil as K
    import oracle
    f = oracle.parse_footer(data[-61:], len(data))
    assert f is not None and f["table_format"] >= N.PBL_TABLE_PEBBLEV6
    ck = f["checksum_type"]
    st, rows = oracle.kv_block_col(oracle.table_block(data, f["metaindex"], ck))
    assert st == 0 and b"pebble.range_key" not in dict(rows)
    foff, flen = f["footer"]
    body = bytearray(data[:foff])
    old = data[foff: foff + flen]

    def put(block):
        off = len(body)
        body.extend(block + b"\0")
        body.extend(oracle.block_checksum(ck, block + b"\0").to_bytes(4, "little"))
        return off, len(block)

    h = put(block_of_spans(spans) if block is None else block)
    entries = dict(rows)
    entries[b"pebble.range_key"] = K._uvarint(h[0]) + K._uvarint(h[1])
    mh = put(K.kv_block(sorted(entries.items())))
    ih = f["index"]
    foot = bytearray(flen)
    foot[0] = old[0]
    hs = K._uvarint(mh[0]) + K._uvarint(mh[1]) + K._uvarint(ih[0]) + K._uvarint(ih[1])
    foot[1:1 + len(hs)] = hs
    co = flen - 16
    keep = co - 4 if f["table_format"] >= N.PBL_TABLE_PEBBLEV7 else co
    foot[keep:] = old[keep:]
    c = oracle.lib().orc_crc32c_update(0, bytes(foot[:co]), co)
    rest = bytes(foot[co + 4:])
    c = oracle.lib().orc_crc32c_update(c, rest, len(rest))
    foot[co:co + 4] = (((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(body + foot)
