"""Helpers of the whole-read-path tests (tests/test_read_histories.py,
tests/test_read_histories_gpu.py; DESIGN.md §3.16, "Tests").

`History` is a flat list of writes with sequence numbers.  `tables()` deals it
into tables under a layout: points as row blocks, tombstones and range keys
fragmented (rangedelutil.fragment) into a row range-del block and a keyspan
block, all decoded on the device, or laid out as host arrays for the CPU suite.
`read_host_forms()` is `pebble_amd.visible.read()`'s composition over the host
forms only.  `expected_read()` is the whole-path model, stated over the flat
list of writes from Iterator's documented behaviour; it calls no host form.
`interleave()` turns points and spans into the combined forward stream that the
reference's iter_histories record (tests/golden/iter_histories.json pins all
three)."""
import functools
import json
import os
import struct

import rangekeyutil as RK
from mergeutil import C, D, T, crdb_key
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare
from pebble_amd.rowblk import Writer
from rangedelutil import brute_cover, fragment, run_block as rd_block, run_host as rd_host, run_kvs
from scanutil import result_kvs
from visibleutil import DEL, MAX, MERGE, SET, SINGLEDEL, expected_visible, host_from_blocks, tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iter_histories.json")
SEQ0 = 10  # base.SeqNumStart: the first sequence number a new database hands out
LAYOUTS = ("one", "per_batch", "dealt")
MAX_TABLES = 16  # merge and the sets take 16 runs
POINT_KINDS = {"set": SET, "del": DEL, "singledel": SINGLEDEL, "merge": MERGE}
OBSOLETE = N.PBL_KV_OBSOLETE


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def b(s):
    return None if s is None else s.encode("latin-1")


def alpha(n):
    """testkeys.Alpha(n) in order: every string of 1..n letters a-z, lexicographically."""
    out = []

    def rec(p):
        for c in "abcdefghijklmnopqrstuvwxyz":
            out.append(p + c)
            if len(p) + 1 < n:
                rec(p + c)
    rec("")
    return out


# ---- the history ------------------------------------------------------------------------------------------
class History:
    """points [(key, seq, kind, value, batch)], tombs [(start, end, seq, batch)],
    rks [(start, end, seq, kind, suffix, value, batch)].  `write(batch)` gives
    each op of a batch the next sequence number, as a committed batch does;
    an op is (name, field, ...) in bytes with the names of runBatchDefineCmd."""

    def __init__(self, comparer=T):
        self.comparer, self.points, self.tombs, self.rks = comparer, [], [], []
        self.seq, self.n_batches = SEQ0, 0

    def write(self, ops):
        bt = self.n_batches
        self.n_batches += 1
        for op in ops:
            name, f, s = op[0], op[1:], self.seq
            self.seq += 1
            if name in POINT_KINDS:
                self.points.append((f[0], s, POINT_KINDS[name], f[1] if len(f) > 1 else b"", bt))
            elif name == "del-range":
                self.tombs.append((f[0], f[1], s, bt))
            elif name == "range-key-set":
                self.rks.append((f[0], f[1], s, RK.SET, f[2], f[3] if len(f) > 3 else b"", bt))
            elif name == "range-key-unset":
                self.rks.append((f[0], f[1], s, RK.UNSET, f[2], b"", bt))
            elif name == "range-key-del":
                self.rks.append((f[0], f[1], s, RK.DEL, b"", b"", bt))
            else:
                raise AssertionError(op)
        return self

    @classmethod
    def from_fixture(cls, section, n_writes):
        h = cls(T)
        for w in section["writes"][:n_writes]:
            if "populate" in w:  # runPopulateCmd: every key of Alpha(keylen), each timestamp in order, value = key
                p = w["populate"]
                keys = [(p["prefix"] + k + "@%d" % ts).encode() for k in alpha(p["keylen"]) for ts in p["timestamps"]]
                h.write([("set", k, k) for k in keys])
            else:
                h.write([tuple([op[0]] + [b(x) for x in op[1:]]) for op in w["ops"]])
        return h

    @classmethod
    def from_define(cls, define, kinds, comparer=D):
        """An option-less, points-only `define` of testdata/iterator: explicit sequence numbers, a batch per KV."""
        h = cls(comparer)
        for i, (k, seq, kind, v) in enumerate(define):
            h.points.append((b(k), seq, kinds[kind], b(v), i))
        h.n_batches = len(define)
        return h


def _ck(comparer):
    return functools.cmp_to_key(lambda x, y: key_compare(comparer, x, y))


def _sorted_points(points, comparer):
    ck = _ck(comparer)
    return sorted(points, key=lambda p: (ck(p[0]), -p[1]))


# ---- the tables -------------------------------------------------------------------------------------------
def row_block(kvs, restart=4):
    w = Writer(restart)
    for kv in kvs:
        w.add(kv[0], kv[1], kv[2])
    return w.finish()


class HistoryTable:
    """What read() needs of a table (comparer, scan, range_dels, range_keys) over
    some of a history's writes, and the same inputs as host arrays (`points_host`,
    `rd_host`, `rk_host`): to_host() of the device's decode with `device`, laid
    out in Python without.  `obsolete`: the sequence numbers of the point KVs
    that carry PBL_KV_OBSOLETE: those under a newer KV of the same user key in
    this table with no MERGE above them (what a table's writer marks)."""

    def __init__(self, points, tombs, rks, comparer, device, per_block, restart=4, mark_obsolete=False):
        self.cmp = comparer
        pts = _sorted_points(points, comparer)
        self.obsolete = set()
        kvs = []
        for j, p in enumerate(pts):
            first = j
            while first > 0 and key_compare(comparer, pts[first - 1][0], p[0]) == 0:
                first -= 1
            obs = mark_obsolete and first < j and all(q[2] != MERGE for q in pts[first:j])
            if obs:
                self.obsolete.add(p[1])
            kvs.append((p[0], tr(p[1], p[2]), p[3], OBSOLETE if obs else 0))
        blocks = [kvs[i: i + per_block] for i in range(0, len(kvs), per_block)] or [[]]
        self.rd_kvs = run_kvs([(s, e, q) for s, e, q, _ in tombs], comparer)
        self.rk_spans = [(s, e, [(tr(k[0], k[1]), k[2], k[3]) for k in ks])
                         for s, e, ks in fragment([(s, e, [(q, kind, sfx, v)]) for s, e, q, kind, sfx, v, _ in rks], comparer)]
        self.d = self.rd = self.rk = None
        if device:
            import torch
            from pebble_amd.batch import BlockBatch, decode
            from pebble_amd.keyspan import decode as keyspan_decode
            one = lambda blks: BlockBatch.from_blocks(blks, "cuda", N.PBL_FMT_ROW, 0)  # noqa: E731
            self.d = decode(one([row_block(blk, restart) for blk in blocks]))
            flags = [kv[3] for kv in kvs]
            if any(flags):
                self.d.kv_flags[: len(flags)] |= torch.tensor(flags, dtype=torch.uint8, device="cuda")
            self.points_host = self.d.to_host()
            if self.rd_kvs:
                self.rd = decode(one([rd_block(self.rd_kvs)]))
            if self.rk_spans:
                self.rk = keyspan_decode(one([RK.run_block(self.rk_spans)]), extras=True)
            self.rd_host = self.rd.to_host() if self.rd is not None else None
            self.rk_host = self.rk.to_host() if self.rk is not None else None
        else:
            from pebble_amd.keyspan import decode_host
            self.points_host = host_from_blocks(blocks)
            self.rd_host = rd_host(self.rd_kvs) if self.rd_kvs else None
            self.rk_host = decode_host([RK.run_block(self.rk_spans)], extras=True) if self.rk_spans else None

    def comparer(self):
        return self.cmp

    def scan(self, lowers, uppers, hide_obsolete_points=False):
        from pebble_amd.scan import scan
        return scan(self.d, lowers, uppers, comparer=self.cmp, hide_obsolete_points=hide_obsolete_points)

    def range_dels(self):
        return self.rd

    def range_keys(self):
        return self.rk


def deal(history, layout, n_tables=3):
    """Per table (points, tombs, rks).  "one": the whole history; "per_batch": a
    table per batch, folded to at most MAX_TABLES; "dealt": the writes in
    sequence-number order dealt round-robin to `n_tables` tables."""
    if layout == "one":
        return [(history.points, history.tombs, history.rks)]
    if layout == "per_batch":
        n = max(1, min(history.n_batches, MAX_TABLES))
        pick = lambda xs, i: [x for x in xs if x[-1] % n == i]  # noqa: E731
        return [(pick(history.points, i), pick(history.tombs, i), pick(history.rks, i)) for i in range(n)]
    assert layout == "dealt" and n_tables <= MAX_TABLES
    seqs = sorted([p[1] for p in history.points] + [t[2] for t in history.tombs] + [r[2] for r in history.rks])
    at = {s: i % n_tables for i, s in enumerate(seqs)}
    return [([p for p in history.points if at[p[1]] == i], [t for t in history.tombs if at[t[2]] == i],
             [r for r in history.rks if at[r[2]] == i]) for i in range(n_tables)]


def tables(history, layout, device=False, per_block=64, n_tables=3, mark_obsolete=False):
    """The history's tables under a layout.  A table may be empty of points (one
    empty row block), of tombstones or of range keys (None)."""
    return [HistoryTable(p, t, r, history.comparer, device, per_block, (1, 4, 16)[i % 3], mark_obsolete)
            for i, (p, t, r) in enumerate(deal(history, layout, n_tables))]


# ---- read() over the host forms -------------------------------------------------------------------------
def _status_names(mask):
    return ", ".join(N.STATUS_NAMES.get(x, str(x)) for x in range(32) if mask >> x & 1)


def read_host_forms(tabs, lowers, uppers, *, snapshot=MAX, hide_obsolete_points=False, keep_operands=False,
                    mask_suffix=None):
    """`pebble_amd.visible.read(..., with_range_keys=True)` over the host forms
    only, in read()'s order: scan_host per table, merge_host, the range-deletion
    set and cover at the snapshot, the range-key set at the snapshot, its clip to
    the ranges, the mask stored into the cover, visible_host.  Returns
    ((result dict, src_kv, n_src), clipped range-key batch dict)."""
    from pebble_amd import rangedel, rangekey
    from pebble_amd.merge import merge_host
    from pebble_amd.scan import scan_host
    from pebble_amd.visible import visible_host
    comparer = tabs[0].comparer()
    hosts = [scan_host(t.points_host, lowers, uppers, comparer=comparer, hide_obsolete_points=hide_obsolete_points)[0]
             for t in tabs]
    merged = merge_host(hosts, comparer=comparer)[0]
    cover = None
    rds = [t.rd_host for t in tabs if t.rd_host is not None]
    if rds:
        rset = rangedel.build_set_host(rds, comparer, snapshot)
        assert not rset["status_mask"], "range deletions: " + _status_names(rset["status_mask"])
        cover, st = rangedel.cover_host(rds, merged, comparer, snapshot)
        assert st == 0
    rk_set = rangekey.build_set_host([t.rk_host for t in tabs if t.rk_host is not None], comparer, snapshot)
    assert not rk_set["status_mask"], "range keys: " + _status_names(rk_set["status_mask"])
    rk_batch = rangekey.clip_host(rk_set, lowers, uppers, comparer)
    if mask_suffix is not None and rk_set["n_kv"]:
        cover = rangekey.mask_set_host(rk_set, merged, comparer, mask_suffix, cover=cover)
    return visible_host(merged, comparer=comparer, snapshot=snapshot, keep_operands=keep_operands, cover=cover), rk_batch


def result_points(r, q):
    """[(key, trailer, value)] of range q of a read result in to_host()'s layout."""
    return [x[:3] for x in result_kvs(r, q)]


def result_spans(rk, q):
    """[(start, end, [(trailer, suffix, value)])] of range q of a clipped range-key batch."""
    return RK.spans_of_host(rk, q)


# ---- the whole-path model ---------------------------------------------------------------------------------
def expected_read(history, lowers, uppers, snapshot=MAX, mask_suffix=None, comparer=None, keep_operands=False,
                  hidden=()):
    """What an Iterator over the history's writes returns going forward, per range
    [lower, upper) (None = unbounded; an empty or inverted range holds nothing),
    at `snapshot`: (points per range [(key, trailer, value)], spans per range
    [(start, end, [(trailer, suffix, value)])]).  Stated over the flat list of
    writes; the parts are the Python statements of the single rules:

      1. a point KV is gone when a del-range visible at the snapshot with a larger
         sequence number covers its key (rangedelutil.brute_cover), or, with a
         mask suffix, when the range keys visible at the snapshot mask its key
         (rangekeyutil.expected_masked: Iterator's RangeKeyMasking; a key without
         a suffix is never masked).  A gone KV is gone for every later rule: it
         neither shadows an older version nor feeds or ends a MERGE chain;
      2. of the rest, per user key the newest version below the snapshot, deleted
         keys dropped, MERGE chains folded (visibleutil.expected_visible);
      3. the range keys: coalesced and defragmented at the snapshot
         (rangekeyutil.expected_spans), truncated to the range (clip_spans).

    `hidden`: sequence numbers of point KVs a scan with hide_obsolete_points
    drops before anything else."""
    comparer = history.comparer if comparer is None else comparer
    pts = [p for p in _sorted_points(history.points, comparer) if p[1] not in hidden]
    tombs = [(s, e, q) for s, e, q, _ in history.tombs]
    runs = [[(s, e, [(tr(q, kind), sfx, v)])] for s, e, q, kind, sfx, v, _ in history.rks]
    spans = RK.expected_spans(runs, comparer, snapshot)
    gone = {}
    out_p, out_s = [], []
    for lo, up in zip(lowers, uppers):
        if lo is not None and up is not None and key_compare(comparer, lo, up) >= 0:
            out_p.append([])
            out_s.append([])
            continue
        kvs = []
        for k, q, kind, v, _ in pts:
            if (lo is not None and key_compare(comparer, k, lo) < 0) or (up is not None and key_compare(comparer, k, up) >= 0):
                continue
            if k not in gone:
                gone[k] = (brute_cover(tombs, k, comparer, snapshot),
                           mask_suffix is not None and RK.expected_masked(runs, k, comparer, mask_suffix, snapshot))
            if gone[k][1] or gone[k][0] > q:
                continue
            kvs.append((k, tr(q, kind), v))
        (st, res), = expected_visible(host_from_blocks([kvs]), comparer, snapshot, keep_operands)
        assert st == 0
        out_p.append([x[:3] for x in res])
        out_s.append(RK.clip_spans(spans, lo, up, comparer))
    return out_p, out_s


# ---- the combined stream ----------------------------------------------------------------------------------
def interleave(points, spans, lower, start, comparer=T):
    """The combined forward stream of an Iterator with KeyTypes = points and
    ranges, bounded to a range, after First() (`start` None) or SeekGE(start):
    [(key, value or None, span or None)], span = (start, end, [(suffix, value)]).
    `points`: the visible [(key, value)] of the range in order; `spans`: the
    range keys truncated to the range.  The rules (iterator.go on
    IterKeyTypePointsAndRanges, HasPointAndRange and RangeBounds;
    internal/keyspan/interleaving_iter.go's file comment; range_keys.go):

      - there is a position at every visible point;
      - there is a position at the start of every span, as truncated to the
        bounds, when no point sits exactly there (the span's start key is
        interleaved as a key of its own, HasPointAndRange = (false, true));
      - every position reports the span that covers it, with the span's
        truncated bounds and its sets in suffix order;
      - SeekGE(K) seeks to max(K, lower); the stream begins at the first position
        at or after that key, and the key itself is a position when a span covers
        it and no point equals it (a span that straddles the seek key is
        interleaved at the seek key).  The span is still reported with its
        truncated start and end, not cut to the seek key."""
    cmp = lambda x, y: key_compare(comparer, x, y)  # noqa: E731
    pos = [(k, v) for k, v in points]
    for s, _, _ in spans:
        if not any(cmp(k, s) == 0 for k, _ in points):
            pos.append((s, None))
    if start is not None:
        if lower is not None and cmp(start, lower) < 0:
            start = lower
        if any(cmp(s, start) <= 0 and cmp(start, e) < 0 for s, e, _ in spans) and not any(cmp(k, start) == 0 for k, _ in pos):
            pos.append((start, None))
        pos = [p for p in pos if cmp(p[0], start) >= 0]
    pos.sort(key=lambda p: _ck(comparer)(p[0]))
    out = []
    for k, v in pos:
        over = [(s, e, [(sfx, val) for _, sfx, val in ks]) for s, e, ks in spans if cmp(s, k) <= 0 and cmp(k, e) < 0]
        assert len(over) <= 1
        out.append((k, v, over[0] if over else None))
    return out


def recorded(lines):
    """A segment's parsed lines in interleave()'s form; None = exhausted."""
    return [None if ln is None else (b(ln[0]), b(ln[1]), None if ln[2] is None else
                                     (b(ln[2][0]), b(ln[2][1]), [(b(s), b(v)) for s, v in ln[2][2]])) for ln in lines]


def replay(points, spans, lower, start, n, comparer=T):
    """The first n lines of the stream: `first` / `seek-ge` and n - 1 `next`."""
    stream = interleave([(k, v) for k, _, v in points], spans, lower, start, comparer)
    return [stream[i] if i < len(stream) else None for i in range(n)]


def groups(g):
    """The fixture's segments grouped by (section, n_writes, mask_suffix): one read() per group, a range per segment."""
    out = {}
    for s in g["segments"]:
        out.setdefault((s["section"], s["n_writes"], s["mask_suffix"]), []).append(s)
    return sorted(out.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2] or ""))


# ---- generated histories ----------------------------------------------------------------------------------
def key_of(comparer, i, version, form=None):
    """User key number i (ascending in i) with version number `version` (0 = none,
    larger = newer = sorts first).  crdb versions take three byte forms: 9 bytes
    (wall), 13 bytes with a zero logical (equal to the 9-byte form as a point
    version, another suffix as a range-key suffix), 13 bytes with a logical."""
    if comparer == T:
        return b"k%04d" % i + (b"@%d" % version if version else b"")
    if comparer == C:
        p = b"k%04d" % i
        if not version:
            return crdb_key(p)
        form = (i + version) % 3 if form is None else form
        return (crdb_key(p, version), crdb_key(p, version, 0), crdb_key(p, version, 7))[form]
    return b"k%04d" % i + (b"#%02d" % (99 - version) if version else b"")


def suffix_of(comparer, version, form=0):
    if not version:
        return b""
    if comparer == T:
        return b"@%d" % version
    if comparer == C:
        w = struct.pack(">Q", version)
        return (w + b"\x09", w + bytes(4) + b"\x0d", w + struct.pack(">I", 7) + b"\x0d")[form % 3]
    return b"#%02d" % (99 - version)


def bound_of(comparer, i):
    return crdb_key(b"k%04d" % i) if comparer == C else b"k%04d" % i


def random_history(rng, comparer, n_keys, n_ops, n_batches, versions=4, p_range=0.08):
    """n_ops writes over n_keys user-key prefixes with `versions` versions each, in
    n_batches batches: mostly point writes (set, merge, del, singledel), some
    del-range and range-key-set / -unset / -del over short stretches of the key
    space, suffixes and values from small pools, so that versions, tombstones
    and spans collide."""
    h = History(comparer)
    per = max(1, n_ops // n_batches)
    ops = []
    for i in range(n_ops):
        x = rng.random()
        if x < p_range:
            a = rng.randrange(n_keys)
            lo, hi = bound_of(comparer, a), bound_of(comparer, a + 1 + rng.randrange(max(1, n_keys // 6)))
            y = rng.random()
            v = rng.randrange(versions + 1)
            if y < 0.3:
                ops.append(("del-range", lo, hi))
            elif y < 0.8:
                ops.append(("range-key-set", lo, hi, suffix_of(comparer, v, rng.randrange(3)), b"rv%d" % rng.randrange(2)))
            elif y < 0.9:
                ops.append(("range-key-unset", lo, hi, suffix_of(comparer, v, rng.randrange(3))))
            else:
                ops.append(("range-key-del", lo, hi))
        else:
            k = key_of(comparer, rng.randrange(n_keys), rng.randrange(versions + 1), rng.randrange(3))
            name = rng.choice(("set", "set", "set", "merge", "merge", "merge", "del", "singledel"))
            ops.append((name, k, b"%s%d;" % (name[:1].encode(), i)) if name in ("set", "merge") else (name, k))
        if len(ops) == per and h.n_batches < n_batches - 1:
            h.write(ops)
            ops = []
    h.write(ops)
    return h


def dense_history(comparer, n_keys, versions=(3,)):
    """n_keys distinct user keys, one SET each, in one batch: a result of exactly n_keys KVs in an unbounded range."""
    h = History(comparer)
    return h.write([("set", key_of(comparer, i, versions[i % len(versions)]), b"v%d" % i) for i in range(n_keys)])
