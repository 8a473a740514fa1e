"""Helpers of the compaction-view tests (tests/test_compact.py,
tests/test_compact_gpu.py).

`expected_compact` is a third statement of include/pebble_amd.h's rules,
written from the reference's text (internal/compact/iterator.go) and
independent of both implementations: it cuts a block into groups of equal user
keys, a group into segments of equal snapshot stripe, and settles each segment
on its own with list operations (no cursor over the block, no state machine).
The fixture (tests/golden/compact_iter.json) is the reference's own recorded
behaviour."""
import json
import os

import numpy as np

from mergeutil import BAD, C, D, T, crdb_key  # noqa: F401
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare
from pebble_amd.rowblk import make_trailer
from scanutil import ARRAYS, TOTALS, result_kvs
from visibleutil import host_from_blocks  # noqa: F401

DEL, SET, MERGE, SINGLEDEL, SETWITHDEL, DELSIZED = 0, 1, 2, 7, 18, 23
KINDS = (DEL, SET, MERGE, SINGLEDEL, SETWITHDEL, DELSIZED)
TOMBS = (DEL, SINGLEDEL, DELSIZED)
VALUED = (SET, MERGE, SETWITHDEL)
HANDLES = N.PBL_KV_VALBLK_HANDLE | N.PBL_KV_BLOB_HANDLE
CORRUPT = N.PBL_CORRUPT_BOUNDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact_iter.json")
COUNTERS = ("n_missized", "n_ineffectual", "n_nondeterministic")


def tr(seq, kind=SET):
    return make_trailer(seq, kind)


def uvarint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def read_uvarint(b):
    """The value when b is exactly one uvarint (binary.Uvarint with n == len(b)), else None."""
    x = 0
    for i, c in enumerate(b[:10]):
        if i == 9 and c > 1:
            return None
        x |= (c & 0x7F) << (7 * i)
        if c < 0x80:
            return x if i + 1 == len(b) else None
    return None


def stripe_of(snapshots, seq):
    return sum(1 for s in snapshots if s <= seq)


class _Block:
    def __init__(self):
        self.results, self.miss, self.ineff, self.nondet = [], 0, 0, 0
        self.unsupported, self.corrupt, self.events = False, False, set()


def _segment(B, kvs, kv0, grp, lo, hi, stripe, elide, bottommost):
    """Settle the segment grp[lo:hi] (indices into kvs) of the group grp."""
    elid = elide and stripe == 0
    low = bottommost and stripe == 0
    at = lo
    while at < hi:
        head = grp[at]
        key, t, val, fl = kvs[head]
        kind, seq = t & 0xff, t >> 8
        rest = [kvs[x][1] & 0xff for x in grp[at + 1: hi]]  # the kinds after the head, to the segment's end
        pinned = int((at == lo and lo > 0) or (elide and kind in TOMBS and stripe != 0))

        def emit(k, s, value, n_src=1):
            B.results.append((key, tr(s, k), value, fl & HANDLES, kv0 + head, n_src, pinned))

        if kind == DEL or (kind == DELSIZED and elid):
            if not elid:
                emit(DEL, seq, b"")
            return
        if kind == SETWITHDEL:
            emit(SETWITHDEL, 0 if low else seq, val)
            return
        if kind == SET:
            with_del = any(k in TOMBS for k in rest)
            B.events.add("set+del" if with_del else "set")
            emit(SETWITHDEL if with_del else SET, 0 if low else seq, val)
            return
        if kind == MERGE:
            stop = next((n for n, k in enumerate(rest) if k != MERGE), None)  # the first KV that is no MERGE
            ops = [head] + (grp[at + 1: hi] if stop is None else grp[at + 1: at + 1 + stop])
            out = SET if low else MERGE
            if stop is not None and rest[stop] in TOMBS:
                out = SETWITHDEL
            elif stop is not None:
                ops.append(grp[at + 1 + stop])
                out = SET
            B.events.add("merge->%d" % out)
            if len(ops) > 1 and any(kvs[x][3] & HANDLES for x in ops):
                B.unsupported = True
            emit(out, 0 if low else seq, b"".join(kvs[x][2] for x in reversed(ops)), len(ops))
            return
        if kind == SINGLEDEL:
            more = 0
            while more < len(rest) and rest[more] == SINGLEDEL:
                more += 1
            B.ineff += more  # every further SINGLEDEL met makes the one before ineffectual
            decider = rest[more] if more < len(rest) else None
            if decider is None:
                if elid:
                    B.ineff += 1
                else:
                    emit(SINGLEDEL, seq, b"")
                B.events.add("sd end")
                return
            if decider in (SET, MERGE):
                after = at + 1 + more + 1  # the KV after the consumed one, in the group
                if after < len(grp) and (kvs[grp[after]][1] & 0xff) in VALUED:
                    B.nondet += 1
                B.events.add("sd consumes")
                at = after
                continue
            if decider != SETWITHDEL:
                B.ineff += 1
            if not elid:
                emit(DEL, seq, b"")
            B.events.add("sd->del")
            return
        # DELSIZED, not elided
        held, out = val, DELSIZED
        for x in grp[at + 1: hi]:
            k2, v2 = kvs[x][1] & 0xff, kvs[x][2]
            expected = None
            if held:
                expected = read_uvarint(held)
                if expected is None:
                    B.corrupt = True
            if k2 in TOMBS:
                if held:
                    B.miss += 1
                held = v2 if k2 == DELSIZED else b""
                if k2 != DELSIZED:
                    out = DEL
                    break
            elif not held:
                out = DEL
                break
            else:
                held = b""
                if len(kvs[x][0]) + len(v2) != expected:
                    B.miss += 1
                    out = DEL
                    break
        B.events.add("ds->%d%s" % (out, "+v" if held else ""))
        emit(out, seq, held)
        return


def expected_compact(h, comparer, snapshots=(), elide=False, bottommost=False, events=None):
    """Per result block (status, [(key, trailer, value, flags, src_kv, n_src, pinned)], (missized, ineffectual,
    nondeterministic))."""
    snapshots = sorted(snapshots)
    out = []
    for q in range(len(h["blk_status"])):
        st = int(h["blk_status"][q])
        kvs = result_kvs(h, q) if st == 0 else []
        kv0 = int(h["blk_kv_base"][q])
        same = [key_compare(comparer, kvs[j][0], kvs[j + 1][0]) for j in range(len(kvs) - 1)]
        if any(c > 0 or (c == 0 and kvs[j][1] >> 8 <= kvs[j + 1][1] >> 8) for j, c in enumerate(same)):
            st = N.PBL_INVALID_ARG
        elif any((t & 0xff) not in KINDS or f & N.PBL_KV_INVALID_KEY for _, t, _, f in kvs):
            st = N.PBL_UNSUPPORTED
        B = _Block()
        if st == 0 and kvs:
            starts = [0] + [j + 1 for j, c in enumerate(same) if c != 0] + [len(kvs)]
            for a, b in zip(starts, starts[1:]):
                grp = list(range(a, b))
                stripes = [stripe_of(snapshots, kvs[x][1] >> 8) for x in grp]
                cuts = [0] + [n for n in range(1, len(grp)) if stripes[n] != stripes[n - 1]] + [len(grp)]
                for lo, hi in zip(cuts, cuts[1:]):
                    _segment(B, kvs, kv0, grp, lo, hi, stripes[lo], elide, bottommost)
            if B.unsupported:
                st = N.PBL_UNSUPPORTED
            elif B.corrupt:
                st = CORRUPT
        if events is not None and st == 0:
            events |= B.events
        out.append((st, B.results, (B.miss, B.ineff, B.nondet)) if st == 0 else (st, [], (0, 0, 0)))
    return out


def assert_compact_is(res, h, comparer, snapshots, elide, bottommost, ctx="", events=None):
    """A result dict (compact_host's layout) against expected_compact()."""
    r = res["batch"]
    exp = expected_compact(h, comparer, snapshots, elide, bottommost, events)
    n = len(exp)
    assert len(r["blk_status"]) == n and len(r["blk_kv_base"]) == n + 1, ctx
    bad, mask = 0, 0
    for q, (st, e, counts) in enumerate(exp):
        assert int(r["blk_status"][q]) == st, (ctx, q, int(r["blk_status"][q]), st)
        if st:
            bad += 1
            mask |= 1 << st
        kv0 = int(r["blk_kv_base"][q])
        got = result_kvs(r, q)
        assert len(got) == len(e), (ctx, q, len(got), len(e), [(g[0], g[1] >> 8, g[1] & 0xff) for g in got],
                                    [(x[0], x[1] >> 8, x[1] & 0xff) for x in e])
        for j, (g, x) in enumerate(zip(got, e)):
            assert g == x[:4], (ctx, q, j, (g[0], g[1] >> 8, g[1] & 0xff, g[2][:20], g[3]),
                                (x[0], x[1] >> 8, x[1] & 0xff, x[2][:20], x[3]))
        for name, col in (("src_kv", 4), ("n_src", 5), ("pinned", 6)):
            assert np.asarray(res[name][kv0: kv0 + len(e)]).astype(np.uint64).tolist() == [x[col] for x in e], (ctx, q, name)
        assert tuple(int(res[c][q]) for c in COUNTERS) == counts, (ctx, q, [int(res[c][q]) for c in COUNTERS], counts)
    assert int(r["blk_kv_base"][n]) == r["n_kv"] == sum(len(e) for _, e, _ in exp), ctx
    assert int(r["blk_key_base"][n]) == r["key_bytes_total"] == len(r["key_bytes"]), ctx
    assert int(r["blk_val_base"][n]) == r["val_bytes_total"] == len(r["val_bytes"]), ctx
    assert r["n_bad_blocks"] == bad and r["status_mask"] == mask, ctx
    assert not r["blk_rst_base"].any() and r["n_restarts"] == 0, ctx
    return exp


def assert_same(a, b, ctx=""):
    """Two result dicts: every array, total, per-KV output and counter, exactly."""
    ra, rb = a["batch"], b["batch"]
    for k in ARRAYS + ("entry_off", "tiering_span_id", "tiering_attr"):
        x, y = ra.get(k), rb.get(k)
        assert (x is None) == (y is None), (ctx, k)
        if x is not None:
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k)
    for k in TOTALS:
        assert int(ra[k]) == int(rb[k]), (ctx, k, ra[k], rb[k])
    for k in ("src_kv", "n_src", "pinned") + COUNTERS:
        x, y = np.asarray(a[k]).astype(np.uint64), np.asarray(b[k]).astype(np.uint64)
        assert x.shape == y.shape and (x == y).all(), (ctx, k)


def device_result(res):
    """A CompactResult in compact_host's layout, numpy."""
    u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    return {"batch": res.batch.to_host(), "src_kv": u(res.src_kv, np.uint64), "n_src": u(res.n_src, np.uint32),
            "pinned": res.pinned.cpu().numpy(), "n_missized": u(res.n_missized, np.uint32),
            "n_ineffectual": u(res.n_ineffectual, np.uint32), "n_nondeterministic": u(res.n_nondeterministic, np.uint32)}


# ---- the reference's recorded cases ------------------------------------------------------------------
def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_block(case, kinds):
    return [(k.encode(), tr(s, kinds[kind]), bytes.fromhex(v)) for k, s, kind, v in case["define"]]


def golden_options(case):
    return tuple(case["snapshots"]), case["elide"], case["bottommost"]


def assert_golden(case, kinds, got, pinned, counts, ctx=""):
    """One block's results [(key, trailer, value, flags)], pinned and counters
    against the reference's recorded lines."""
    want = [(k.encode(), tr(s, kinds[kind]), bytes.fromhex(v)) for k, s, kind, v, *_ in case["results"]]
    all_returned = len(got) == len(want)
    if not case["complete"]:  # the recorded commands stop at the last result they asked for
        got, pinned = got[: len(want)], pinned[: len(want)]
    assert [g[:3] for g in got] == want, (ctx, [(g[0], g[1] >> 8, g[1] & 0xff, g[2]) for g in got], case["results"])
    if case["print_pinned"]:
        assert [int(p) for p in pinned] == [r[4] for r in case["results"]], (ctx, "pinned")
    if case["complete"]:
        if case["missized_known"]:
            assert counts[0] == case["missized"], (ctx, "missized", counts[0], case["missized"])
        assert counts[1] == case["ineffectual"], (ctx, "ineffectual", counts[1], case["ineffectual"])
        assert counts[2] == case["nondeterministic"], (ctx, "nondeterministic", counts[2], case["nondeterministic"])
    elif all_returned and case["missized_known"]:
        # every result was returned, so the last head's look-ahead is done and the printed count is the whole count
        assert counts[0] == case["missized"], (ctx, "missized", counts[0], case["missized"])


# ---- the state before a KV, for tests that place a state at a given position ------------------------
STATES = ("seeking", "set looking", "merging", "singledel pending", "singledel pending under elision",
          "delsized holding", "delsized empty", "skipping")


def state_before(kvs, at, snapshots=(), elide=False):
    """The iterator's state when it reaches kvs[at] (one block's KVs, one user
    key's versions around `at` compared by bytes): the walk from the start of
    at's segment, in the words of include/pebble_amd.h."""
    stripe = lambda x: stripe_of(snapshots, kvs[x][1] >> 8)  # noqa: E731
    lo = at
    while lo > 0 and kvs[lo - 1][0] == kvs[at][0] and stripe(lo - 1) == stripe(at):
        lo -= 1
    elid = elide and stripe(at) == 0
    s = "seeking"
    for x in range(lo, at):
        key, t, val, _ = kvs[x]
        k = t & 0xff
        by_value = "delsized holding" if val else "delsized empty"
        if s == "seeking":
            s = {DEL: "skipping", SETWITHDEL: "skipping", SET: "set looking", MERGE: "merging",
                 SINGLEDEL: "singledel pending under elision" if elid else "singledel pending",
                 DELSIZED: "skipping" if elid else by_value}[k]
        elif s == "set looking":
            s = "skipping" if k in TOMBS else s
        elif s == "merging":
            s = s if k == MERGE else "skipping"
        elif s.startswith("singledel pending"):
            s = s if k == SINGLEDEL else "seeking" if k in (SET, MERGE) else "skipping"
        elif s == "delsized holding":
            held = read_uvarint(kvs[x - 1][2])
            s = by_value if k == DELSIZED else "delsized empty" if k in VALUED and len(key) + len(val) == held else "skipping"
        elif s == "delsized empty":
            s = by_value if k == DELSIZED else "skipping"
    return s


# ---- generated inputs -------------------------------------------------------------------------------
WEIGHTED = [SET] * 4 + [MERGE] * 5 + [DEL] * 2 + [SINGLEDEL] * 5 + [SETWITHDEL] * 2 + [DELSIZED] * 5


def user_keys(comparer, n):
    """n distinct user keys in the comparer's order, in the comparer's own key shape."""
    if comparer == C:
        return [crdb_key(b"k%04d" % i, 5 + i % 3) for i in range(n)]
    if comparer == T:
        return [b"k%04d@%d" % (i, 9 - i % 3) for i in range(n)]
    return [b"k%04d" % i for i in range(n)]


def random_block(rng, comparer, n_groups, seq_top=4000):
    """Groups of 1 to 40 versions; DELSIZED values are the next KV's true size,
    a wrong size or empty; other values are 0, a few or 600 bytes."""
    blk = []
    for key in user_keys(comparer, n_groups):
        n = int(rng.integers(1, 41)) if rng.random() < 0.3 else int(rng.integers(1, 7))
        seqs = sorted(rng.choice(np.arange(1, seq_top), size=n, replace=False).tolist(), reverse=True)
        kinds = [WEIGHTED[int(rng.integers(len(WEIGHTED)))] for _ in range(n)]
        vals = []
        for i, k in enumerate(kinds):
            if k in (DEL, SINGLEDEL):
                vals.append(b"")
            elif k == DELSIZED:
                vals.append(None)
            else:
                c = rng.random()
                vals.append(b"" if c < 0.2 else bytes([65 + i % 26]) * 600 if c < 0.3 else b"v%d;" % seqs[i])
        for i, k in enumerate(kinds):
            if k == DELSIZED:
                c = rng.random()
                nxt = len(key) + len(vals[i + 1] or b"") if i + 1 < n else 7
                vals[i] = b"" if c < 0.3 else uvarint(nxt) if c < 0.75 else uvarint(nxt + 1 + int(rng.integers(300)))
        blk += [(key, tr(s, k), v) for s, k, v in zip(seqs, kinds, vals)]
    return blk


def snapshot_list(rng, n, seq_top=4000):
    return sorted(rng.choice(np.arange(1, seq_top + 50), size=n, replace=False).tolist()) if n else []


ALL_EVENTS = {"set", "set+del", "merge->%d" % MERGE, "merge->%d" % SET, "merge->%d" % SETWITHDEL, "sd end", "sd consumes",
              "sd->del", "ds->%d" % DEL, "ds->%d" % DELSIZED, "ds->%d+v" % DELSIZED}


def group(key, kinds, seq_top, vals=None):
    """One key's versions with these kinds, sequence numbers seq_top downwards."""
    vals = vals or [b"" if k in (DEL, SINGLEDEL, DELSIZED) else b"v%d;" % (seq_top - i) for i, k in enumerate(kinds)]
    return [(key, tr(seq_top - i, k), v) for i, (k, v) in enumerate(zip(kinds, vals))]


def status_blocks():
    good = lambda q: (group(b"k%da" % q, [MERGE, MERGE, SET], 30) + group(b"k%db" % q, [SINGLEDEL, SET, DEL, SET], 20)  # noqa: E731
                      + group(b"k%dc" % q, [DELSIZED, SET], 9, [uvarint(3 + len(b"k%dc" % q)), b"abc"]))
    unsorted = [(b"b", tr(2), b"x"), (b"a", tr(1), b"y")]
    equal_seq = [(b"x", tr(2, SET), b"new"), (b"x", tr(2, DEL), b"")]
    kind21 = [(b"a", tr(9), b"ok"), (b"b", tr(8, 21), b"range key set"), (b"c", tr(7), b"ok")]
    handle = [(b"a", tr(9, MERGE), b"op"), (b"a", tr(8, SET), b"\x80handle", N.PBL_KV_VALBLK_HANDLE),
              (b"b", tr(7, SET), b"\x80alone", N.PBL_KV_BLOB_HANDLE)]
    two_uvarints = [(b"a", tr(9, DELSIZED), uvarint(300) + uvarint(1)), (b"a", tr(8, SET), b"v")]
    lone_bad = [(b"a", tr(9, DELSIZED), uvarint(300) + uvarint(1)), (b"b", tr(8, SET), b"never decoded: PBL_OK")]
    blocks = [good(0)]
    for q, b in enumerate((None, unsorted, equal_seq, kind21, handle, two_uvarints, lone_bad, [])):
        blocks += [b, good(q + 1)]
    return blocks


STATUS_EXPECTED = [0, BAD, 0, N.PBL_INVALID_ARG, 0, N.PBL_INVALID_ARG, 0, N.PBL_UNSUPPORTED, 0, N.PBL_UNSUPPORTED, 0, CORRUPT,
                   0, 0, 0, 0, 0]
