"""Helpers of the row-block encoder tests (tests/test_rowenc.py,
tests/test_rowenc_gpu.py).

`model_encode` is a Python statement of include/pebble_amd.h's encoder rules
1-7, sequential like the reference: RawRowWriter.addPoint per KV
(makeAddPointDecisionV3, sstable/rowblk_writer.go:585-774), shouldFlush before
every Add (:1238-1262, FlushGovernor without size classes), a fresh
`pebble_amd.rowblk.Writer` per block.  Its result has the layout of
`pebble_amd.rowenc.encode_host`.  The case list is shared by the host and the
device tests: a case is (name, RowEncOptions, streams); a stream is a list of
(user key, trailer, value[, kv_flags]) in order, or None for a stream that is
not PBL_OK."""
import functools
import json
import os
import random

import numpy as np
import torch

import oracle
from mergeutil import BAD, C, D, T, crdb_key
from pebble_amd import _native as N
from pebble_amd.blockiter import key_compare, key_split
from pebble_amd.batch import Capacity, DecodedBatch
from pebble_amd.rowblk import Writer, kvs_of_block, make_trailer
from pebble_amd.rowenc import RowEncOptions
from visibleutil import host_from_blocks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEL, SET, MERGE, SINGLEDEL, SETWITHDEL, DELSIZED = 0, 1, 2, 7, 18, 23
TOMBSTONES = (DEL, SINGLEDEL, DELSIZED)
ARRAYS = ("blocks", "block_off", "block_len", "block_stream", "block_first_kv", "block_n_kv", "stream_block_base",
          "stream_status", "obsolete")
TOTALS = ("n_blocks", "block_bytes", "n_restarts", "status_mask", "n_bad_streams")


def tr(seq, kind=SET):
    return make_trailer(seq, kind)


def uvarint_len(x):
    n = 1
    while x >= 0x80:
        x >>= 7
        n += 1
    return n


def stream_kvs(host, q):
    return [(kv.user_key, kv.trailer, kv.value, kv.flags) for kv in kvs_of_block(host, q)]


def model_encode(host, opts: RowEncOptions):
    n = len(host["blk_status"])
    low = (opts.target_block_size * opts.block_size_threshold + 99) // 100
    high, ri, cmp = opts.target_block_size, opts.restart_interval, opts.comparer
    blocks, off, lens, bstream, first, nkv, sbb, sst = bytearray(), [], [], [], [], [], [], []
    obsolete = np.zeros(int(host["blk_kv_base"][n]) if n else 0, np.uint8)
    n_restarts = 0
    w = Writer(ri)
    for q in range(n):
        sbb.append(len(off))
        st = int(host["blk_status"][q])
        sst.append(st)
        if st != N.PBL_OK:
            continue
        kv0 = int(host["blk_kv_base"][q])
        kvs = stream_kvs(host, q)
        start = 0

        def flush(end):
            nonlocal start, n_restarts
            b = w.finish()
            off.append(len(blocks))
            lens.append(len(b))
            bstream.append(q)
            first.append(kv0 + start)
            nkv.append(end - start)
            n_restarts += (end - start - 1) // ri + 1
            blocks.extend(b + bytes(-len(b) % 16))
            w.reset()
            start = end

        w.reset()
        prev_obs = False
        for j, (key, trailer, value, flags) in enumerate(kvs):
            kind = trailer & 0xFF
            set_same = obs = False
            max_shared = len(key)
            add_prefix = opts.value_prefix and kind == SET
            if opts.value_prefix:
                max_shared = 0
                if j:
                    pkey, pkind = kvs[j - 1][0], kvs[j - 1][1] & 0xFF
                    sp, sc = key_split(cmp, pkey), key_split(cmp, key)
                    max_shared = sp
                    set_same = kind == SET and pkind == SET and key_compare(cmp, pkey[:sp], key[:sc]) == 0
                    same_user = key_compare(cmp, pkey, key) == 0
                    obs = (same_user and (prev_obs or pkind != MERGE)) or (opts.lowest_level and kind in TOMBSTONES)
                obs = opts.obsolete and (obs or bool(flags & N.PBL_KV_OBSOLETE))
            prev_obs = obs
            ikl, svl = len(key) + 8, len(value) + (1 if add_prefix else 0)
            cnt, est = w.entry_count(), w.estimated_size()
            if cnt and est >= low:
                new = est + ikl + svl + (4 if cnt % ri == 0 else 0) + 4 + uvarint_len(ikl) + uvarint_len(svl)
                if new > high:
                    flush(j)
            w.add_with_optional_value_prefix(key, trailer, obs, value, max_shared, add_prefix,
                                             0x20 if set_same else 0x00, set_same)
            obsolete[kv0 + j] = 1 if obs else 0
        if w.entry_count():
            flush(len(kvs))
    sbb.append(len(off))
    bad = [s for s in sst if s]
    mask = 0
    for s in bad:
        mask |= 1 << s
    return {"blocks": np.frombuffer(bytes(blocks), np.uint8), "block_off": np.array(off, np.uint64),
            "block_len": np.array(lens, np.uint32), "block_stream": np.array(bstream, np.uint32),
            "block_first_kv": np.array(first, np.uint64), "block_n_kv": np.array(nkv, np.uint32),
            "stream_block_base": np.array(sbb, np.uint64), "stream_status": np.array(sst, np.uint32),
            "obsolete": obsolete, "n_blocks": len(off), "block_bytes": len(blocks), "n_restarts": n_restarts,
            "status_mask": mask, "n_bad_streams": len(bad)}


def assert_same(a, b, ctx=""):
    """Every output array and total of two results, exactly."""
    for k in TOTALS:
        assert a[k] == b[k], (ctx, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (ctx, k, x.shape, y.shape)
        if not np.array_equal(x, y):
            at = int(np.nonzero(x != y)[0][0])
            raise AssertionError((ctx, k, at, x[at:at + 8].tolist(), y[at:at + 8].tolist()))


def block_bytes(r, b):
    o = int(r["block_off"][b])
    return bytes(r["blocks"][o:o + int(r["block_len"][b])])


def assert_round_trip(host, r, opts: RowEncOptions, decoded=None, ctx=""):
    """decode(encode(x)) == x: keys, trailers, values and obsolete flags of every
    stream that was encoded, restart flags against rule 6.  `decoded`: the
    blocks of `r` decoded (a to_host() dict); the oracle decodes them otherwise."""
    if decoded is None:
        buf = np.concatenate([np.asarray(r["blocks"], np.uint8), np.zeros(16, np.uint8)])
        decoded = oracle.rowblk_decode_batch(buf, r["block_off"], r["block_len"], opts.decode_flags())
    assert not decoded["status_mask"], (ctx, decoded["status_mask"])
    ri = opts.restart_interval
    for q in range(len(host["blk_status"])):
        b0, b1 = int(r["stream_block_base"][q]), int(r["stream_block_base"][q + 1])
        if int(r["stream_status"][q]) != N.PBL_OK:
            assert b0 == b1, (ctx, q)
            continue
        src = stream_kvs(host, q)
        got, same = [], []
        for b in range(b0, b1):
            kvs = kvs_of_block(decoded, b)
            assert len(kvs) == int(r["block_n_kv"][b]) and int(r["block_stream"][b]) == q, (ctx, b)
            assert int(r["block_first_kv"][b]) == int(host["blk_kv_base"][q]) + len(got), (ctx, b)
            for j, kv in enumerate(kvs):
                assert bool(kv.flags & N.PBL_KV_RESTART) == (j % ri == 0), (ctx, b, j)
            same.append([bool(kv.flags & N.PBL_KV_RESTART_SAMEPFX) for kv in kvs])
            got += kvs
        assert len(got) == len(src), (ctx, q, len(got), len(src))
        kv0 = int(host["blk_kv_base"][q])
        set_same = []
        for j, ((key, trailer, value, _f), kv) in enumerate(zip(src, got)):
            assert (kv.user_key, kv.trailer, kv.value) == (key, trailer, value), (ctx, q, j)
            assert bool(kv.flags & N.PBL_KV_OBSOLETE) == bool(r["obsolete"][kv0 + j]), (ctx, q, j)
            ss = False
            if opts.value_prefix and j and (trailer & 0xFF) == SET and (src[j - 1][1] & 0xFF) == SET:
                p = src[j - 1][0]
                ss = key_compare(opts.comparer, p[:key_split(opts.comparer, p)],
                                 key[:key_split(opts.comparer, key)]) == 0
            set_same.append(ss)
        at = 0
        for flags in same:  # rule 6
            for j, f in enumerate(flags):
                if j % ri == 0:
                    exp = j >= ri and all(set_same[at + j - ri + 1: at + j + 1])
                    assert f == exp, (ctx, q, at + j)
            at += len(flags)


# ---- fixtures --------------------------------------------------------------------
def load_golden():
    with open(os.path.join(GOLDEN, "rowenc.json")) as f:
        return json.load(f)


def hamlet():
    """The 14 data blocks of the reference's h-no-compression table and their
    1710 KVs as one stream: (blocks as bytes, host batch)."""
    with open(os.path.join(GOLDEN, "rowblk_golden.json")) as f:
        g = json.load(f)["h_no_compression"]
    blob = np.fromfile(os.path.join(GOLDEN, "h_no_compression_blocks.bin"), np.uint8)
    off, lens = np.array(g["block_off"], np.uint64), np.array(g["block_len"], np.uint32)
    dec = oracle.rowblk_decode_batch(np.concatenate([blob, np.zeros(16, np.uint8)]), off, lens, 0)
    assert not dec["status_mask"]
    kvs = []
    for b in range(len(off)):
        kvs += stream_kvs(dec, b)
    blocks = [bytes(blob[int(o):int(o) + int(n)]) for o, n in zip(off, lens)]
    return blocks, host_from_blocks([[(k, t, v) for k, t, v, _f in kvs]])


HAMLET_OPTS = RowEncOptions(restart_interval=16, target_block_size=2048, block_size_threshold=90)


# ---- the shared cases ---------------------------------------------------------------
def user_keys(comparer, rng, n):
    """n sorted, distinct user keys whose prefixes repeat."""
    pre = sorted({bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 6))) for _ in range(max(2, n // 3))})
    out = set()
    while len(out) < n:
        p = rng.choice(pre)
        if comparer == T:
            out.add(p if rng.random() < 0.2 else p + b"@%d" % rng.randint(1, 40))
        elif comparer == C:
            out.add(crdb_key(p) if rng.random() < 0.2 else crdb_key(p, rng.randint(1, 40)))
        else:
            out.add(p + bytes(rng.choice(b"xyz") for _ in range(rng.randint(0, 3))))
    return sorted(out, key=functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b)))


def random_stream(rng, comparer, n_keys, max_val=40):
    """A sorted stream: per user key a few versions, sequence numbers descending."""
    kvs = []
    for key in user_keys(comparer, rng, n_keys):
        seq = rng.randint(50, 90)
        for _ in range(rng.choice((1, 1, 1, 2, 3, 5))):
            kind = rng.choice((SET, SET, SET, SET, MERGE, MERGE, DEL, SINGLEDEL, SETWITHDEL, DELSIZED))
            val = b"" if kind in (DEL, SINGLEDEL) else bytes(rng.getrandbits(8) for _ in range(rng.randint(0, max_val)))
            kvs.append((key, tr(seq, kind), val, N.PBL_KV_OBSOLETE if rng.random() < 0.05 else 0))
            seq -= rng.randint(1, 9)
    return kvs


FLAG_SETS = ((False, False, False), (True, False, False), (True, True, False), (True, True, True),
             (True, False, True), (False, False, True))


def opts_of(ri, target, comparer=D, flags=(False, False, False), threshold=90):
    return RowEncOptions(ri, target, threshold, comparer, *flags)


def random_cases(seed=7):
    rng = random.Random(seed)
    out = []
    for comparer in (D, T, C):
        for flags in FLAG_SETS:
            ri = rng.choice((1, 2, 3, 16))
            target = rng.choice((64, 200, 700))
            streams = [random_stream(rng, comparer, rng.randint(1, 40)) for _ in range(3)] + [[]]
            out.append((f"random cmp={comparer} flags={flags} ri={ri} target={target}",
                        opts_of(ri, target, comparer, flags, rng.choice((50, 90, 100))), streams))
    return out


def seq_stream(n, klen=4, vlen=0, seq=9, kind=SET):
    return [(b"%0*d" % (klen, i), tr(seq, kind), b"v" * vlen) for i in range(n)]


def edge_cases():
    """The smallest shapes at which each piece can go wrong (host and device)."""
    V3, V4, V4L = (True, False, False), (True, True, False), (True, True, True)
    out = []
    for ri in (1, 2, 16, 17):  # streams of 0, 1, 2, ri, ri + 1 KVs
        out.append((f"tiny ri={ri}", opts_of(ri, 4096), [seq_stream(n) for n in (0, 1, 2, ri, ri + 1)]))
        out.append((f"tiny v3 ri={ri}", opts_of(ri, 80, D, V3), [seq_stream(n) for n in (0, 1, 2, ri, ri + 1)]))
    # a single KV of 3 x target mid-stream and as the first KV: the low-watermark overshoot
    big = (b"0005x", tr(9), b"B" * 768)
    s = seq_stream(12, vlen=10)
    out.append(("overshoot mid", opts_of(4, 256), [sorted(s + [big])]))
    out.append(("overshoot first", opts_of(4, 256), [[(b"0", tr(9), b"B" * 768)] + s]))
    # internal-key lengths 127 / 128 and 16383 / 16384; stored-value lengths 127 / 128 with and without the prefix byte
    for flags in ((False, False, False), V3):
        ks = [b"k" * n for n in (119, 120, 16375, 16376)]
        out.append((f"varint key edges {flags}", opts_of(2, 100000, D, flags), [[(k, tr(5), b"v") for k in ks]]))
        vs = [(b"a%d" % i, tr(5, kind), b"v" * n) for i, (kind, n) in
              enumerate((k, n) for n in (126, 127, 128) for k in (SET, MERGE))]
        out.append((f"varint value edges {flags}", opts_of(3, 100000, D, flags), [vs]))
    # a shared prefix >= 128
    out.append(("shared >= 128", opts_of(16, 100000), [[(b"p" * 200 + b"%02d" % i, tr(5), b"v") for i in range(5)]]))
    # rule 2's trap: a shorter predecessor's trailer bytes take part
    trap = [(b"k", tr(1, SET), b"a"), (b"k\x01" + b"\x00" * 6 + b"z", tr(7), b"b"), (b"k\x01\x01", tr(0x0101010101, SET), b"c"),
            (b"k\x01\x01\x01", tr(3), b"d")]
    for flags in ((False, False, False), V3):
        out.append((f"trap {flags}", opts_of(16, 4096, D, flags), [trap]))
    # equal user keys at several sequence numbers
    same = [(b"key%d" % (i // 4), tr(40 - i), b"v%d" % i) for i in range(24)]
    out.append(("equal user keys", opts_of(3, 90), [same]))
    out.append(("equal user keys v4", opts_of(3, 90, D, V4), [same]))
    # Split prefixes shorter than the common prefix: the v3 cap bites
    tk = [(b"abcdef@%d" % s, tr(9), b"v") for s in (9, 7, 5, 3)] + [(b"abcdeg@%d" % s, tr(9), b"v") for s in (9, 7)]
    out.append(("testkeys cap", opts_of(16, 4096, T, V3), [tk]))
    out.append(("testkeys no cap", opts_of(16, 4096, T), [tk]))
    ck = [(crdb_key(b"roach", w), tr(9), b"v") for w in (9, 7, 5)] + [(crdb_key(b"roachx", w), tr(9), b"v") for w in (9, 7)]
    out.append(("crdb cap", opts_of(16, 4096, C, V3), [ck]))
    # ri consecutive same-prefix SETs, and ri - 1 of them broken by a DEL: bit 31 on and off
    ri = 4
    run = [(b"pp@%d" % (60 - i), tr(9), b"v") for i in range(3 * ri + 1)]
    broken = list(run)
    broken[ri + 2] = (broken[ri + 2][0], tr(9, DEL), b"")
    out.append(("bit 31 on", opts_of(ri, 4096, T, V3), [run]))
    out.append(("bit 31 off", opts_of(ri, 4096, T, V3), [broken]))
    # a run of same-prefix SETs crossing a block cut: restart 0 stays clear, the first value's prefix byte is set
    out.append(("same prefix across a cut", opts_of(ri, 60, T, V3), [run]))
    # obsolete: MERGE, MERGE, SET, SET on one user key; LOWEST_LEVEL tombstones; a forced head; 300 MERGEs
    mmss = [(b"a", tr(9, MERGE), b"1"), (b"a", tr(8, MERGE), b"2"), (b"a", tr(7), b"3"), (b"a", tr(6), b"4"),
            (b"b", tr(5), b"5")]
    out.append(("obsolete mmss", opts_of(2, 4096, D, V4), [mmss]))
    tomb = [(b"a", tr(9, DEL), b""), (b"b", tr(9, SINGLEDEL), b""), (b"c", tr(9, DELSIZED), b"\x05"), (b"d", tr(9), b"v"),
            (b"d", tr(8, DEL), b"")]
    out.append(("lowest level", opts_of(2, 4096, D, V4L), [tomb, tomb[1:]]))
    out.append(("not lowest level", opts_of(2, 4096, D, V4), [tomb]))
    forced = [(b"a", tr(9, MERGE), b"1", N.PBL_KV_OBSOLETE), (b"a", tr(8, MERGE), b"2"), (b"b", tr(7, MERGE), b"3"),
              (b"b", tr(6, MERGE), b"4")]
    out.append(("forced head", opts_of(2, 4096, D, V4), [forced]))
    out.append(("forced ignored", opts_of(2, 4096, D, V3), [forced]))
    chain = [(b"m", tr(1000 - i, MERGE), b"%d" % i) for i in range(300)] + [(b"m", tr(5), b"s"), (b"m", tr(4), b"t")]
    out.append(("merge chain", opts_of(16, 512, D, V4), [chain, [(b"k", tr(3), b"v")] + chain]))
    # a corrupt input block among good ones
    out.append(("bad stream", opts_of(2, 64), [seq_stream(9), None, seq_stream(5), None]))
    # streams that are not OK and carry KVs, beside good ones: their KVs are stepped over
    out.append(("bad streams with KVs", opts_of(2, 64, D, V4L),
                [Bad(seq_stream(7)), seq_stream(9), Bad(same), same, Bad(seq_stream(300)), seq_stream(5), Bad(tomb)]))
    return out


class Bad(list):
    """A stream that is not PBL_OK but carries KVs (a None stream carries none)."""


def host_of(streams):
    h = host_from_blocks(streams)
    for q, s in enumerate(streams):
        if isinstance(s, Bad):
            h["blk_status"][q] = BAD
    bad = int((h["blk_status"] != 0).sum())
    h["n_bad_blocks"], h["status_mask"] = bad, (1 << BAD) if bad else 0
    return h


def upload(host: dict, device="cuda") -> DecodedBatch:
    """A `DecodedBatch` on `device` from host arrays in `to_host()`'s layout
    (the inverse of `DecodedBatch.to_host()`; the byte buffers get the 16-byte
    readable slack the kernels rely on)."""
    nb = len(host["blk_status"])
    n_kv = int(host["blk_kv_base"][nb]) if nb else 0
    nk, nv = (int(host["blk_key_base"][nb]), int(host["blk_val_base"][nb])) if nb else (0, 0)
    out = DecodedBatch.allocate(nb, Capacity(n_kv, nk, nv, 0), device, entry_off=False, restarts=False)

    def put(dst: torch.Tensor, a, dt):
        a = np.ascontiguousarray(np.asarray(a, dt))
        if a.size:
            dst[: a.size].copy_(torch.from_numpy(a.view({np.uint64: np.int64, np.uint32: np.int32}.get(dt, dt))))

    put(out.trailer, host["trailer"], np.uint64)
    put(out.kv_flags, host["kv_flags"] if host.get("kv_flags") is not None else np.zeros(n_kv, np.uint8), np.uint8)
    put(out.key_off, host["key_off"], np.uint32)
    put(out.val_off, host["val_off"], np.uint32)
    put(out.key_bytes, host["key_bytes"], np.uint8)
    put(out.val_bytes, host["val_bytes"], np.uint8)
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base"):
        put(getattr(out, k), host[k], np.uint64)
    out.blk_rst_base.zero_()
    put(out.blk_status, host["blk_status"], np.uint32)
    tot = N.TotalsC(n_kv, nk, nv, 0, int(host.get("status_mask", 0)), int(host.get("n_bad_blocks", 0)), 0, 0)
    out.totals.copy_(torch.from_numpy(np.frombuffer(bytes(tot), np.uint8).copy()))
    return out
