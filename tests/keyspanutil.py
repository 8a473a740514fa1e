"""Helpers of the keyspan tests (tests/test_keyspan.py, tests/test_keyspan_gpu.py).

`decode_block` is the second statement of include/pebble_amd.h's rule for
columnar keyspan blocks: a Python decoder that works straight from block bytes
and shares nothing with pebble_amd.keyspan.Writer or with the library.  It is
pinned by the reference's own blocks and iterator outputs
(tests/golden/keyspan.json).  `expected` lays its KVs out as `to_host()` does,
with the extra output's arrays, so that device and host results are compared
byte for byte.  `with_range_dels` re-emits a golden columnar table with a
keyspan block of range deletions: no reference table file is columnar and holds
range deletions."""
import json
import os

import numpy as np

from pebble_amd import _native as N
from pebble_amd.keyspan import EXTRA_KEYS, Writer, encode_block

RANGEDEL = 15
KINDS = {"RANGEDEL": 15, "RANGEKEYDEL": 19, "RANGEKEYUNSET": 20, "RANGEKEYSET": 21}
HEADER, BOUNDS, UNSUPPORTED = N.PBL_CORRUPT_COLBLK_HEADER, N.PBL_CORRUPT_BOUNDS, N.PBL_UNSUPPORTED
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyspan.json")
ARRAYS = ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status", "trailer", "kv_flags", "entry_off",
          "key_off", "val_off", "key_bytes", "val_bytes")
TOTALS = ("n_kv", "key_bytes_total", "val_bytes_total", "n_restarts", "status_mask", "n_bad_blocks")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


class _Corrupt(Exception):
    pass


def _uints(blk, off, rows):
    """DecodeUnsafeUints: (get(i), end, base, width)."""
    if rows == 0:
        return (lambda i: 0), off, 0, 0
    if off >= len(blk):
        raise _Corrupt
    enc = blk[off]
    off += 1
    w, delta = enc & 0x7F, bool(enc & 0x80)
    if w not in (0, 1, 2, 4, 8) or (w == 8 and delta):
        raise _Corrupt
    base = 0
    if delta:
        if off + 8 > len(blk):
            raise _Corrupt
        base = int.from_bytes(blk[off:off + 8], "little")
        off += 8
    if w:
        off = (off + w - 1) // w * w
    at = off
    return (lambda i: base + (int.from_bytes(blk[at + i * w: at + (i + 1) * w], "little") if w else 0)), at + rows * w, base, w


def _rawbytes(blk, off, rows):
    """DecodeRawBytes: (offset(i), data start, end)."""
    if rows == 0:
        return (lambda i: 0), off, off
    get, data, base, w = _uints(blk, off, rows + 1)
    if base != 0 or w == 8 or data > len(blk) or data + get(rows) > len(blk):  # DecodeUnsafeOffsets
        raise _Corrupt
    return get, data, data + get(rows)


def decode_block(blk: bytes, synthetic_seq_num: int = 0):
    """(status, [(start, end, trailer, suffix, value, span, row)]) of one block."""
    blk = bytes(blk)
    try:
        if len(blk) < 11:
            raise _Corrupt
        B = int.from_bytes(blk[0:4], "little")
        ncols = int.from_bytes(blk[5:7], "little")
        R = int.from_bytes(blk[7:11], "little")
        if ncols != 5:
            raise _Corrupt
        cols = []
        for c, (typ, rows) in enumerate(((3, B), (2, B), (2, R), (3, R), (3, R))):
            h = 11 + 5 * c
            if h + 5 > len(blk) or blk[h] != typ:
                raise _Corrupt
            start = int.from_bytes(blk[h + 1:h + 5], "little")
            if c == 4:
                nxt = len(blk) - 1
            else:
                if h + 10 > len(blk):
                    raise _Corrupt
                nxt = int.from_bytes(blk[h + 6:h + 10], "little")
            if nxt > len(blk) or start > nxt:
                raise _Corrupt
            if typ == 2:
                get, end, _, _ = _uints(blk, start, rows)
                cols.append((get, None))
            else:
                get, data, end = _rawbytes(blk, start, rows)
                cols.append((get, data))
            if end != nxt:
                raise _Corrupt
    except _Corrupt:
        return HEADER, []
    (boff, bdata), (idx, _), (trl, _), (soff, sdata), (voff, vdata) = cols
    if B < 2:
        return 0, []
    if B > len(blk):
        return BOUNDS, []
    if any(boff(i) > boff(i + 1) for i in range(B)) or any(idx(s) > idx(s + 1) for s in range(B - 1)) or idx(B - 1) > R:
        return BOUNDS, []
    empty = [idx(s) == idx(s + 1) for s in range(B - 1)]
    if empty[-1] or any(a and b for a, b in zip(empty, empty[1:])):
        return BOUNDS, []
    if any(soff(j) > soff(j + 1) or voff(j) > voff(j + 1) for j in range(idx(0), idx(B - 1))):
        return BOUNDS, []
    if soff(idx(B - 1)) > soff(R) or voff(idx(B - 1)) > voff(R):  # the last slice that is output, past its column
        return BOUNDS, []
    out = []
    for s in range(B - 1):
        start, end = blk[bdata + boff(s): bdata + boff(s + 1)], blk[bdata + boff(s + 1): bdata + boff(s + 2)]
        for j in range(idx(s), idx(s + 1)):
            t = trl(j)
            if synthetic_seq_num:
                t = synthetic_seq_num << 8 | (t & 0xFF)
            out.append((start, end, t, blk[sdata + soff(j): sdata + soff(j + 1)], blk[vdata + voff(j): vdata + voff(j + 1)],
                        s, j))
    if sum(len(x[0]) for x in out) > 0xFFFFFFFF or sum(len(x[1]) for x in out) > 0xFFFFFFFF:
        return UNSUPPORTED, []
    return 0, out


def expected(blocks, synthetic_seq_num: int = 0, extras: bool = True) -> dict:
    """The decode of the blocks in `to_host()`'s layout (with the extra output's
    arrays), from decode_block."""
    nb = len(blocks)
    t, eo, sp = [], [], []
    offs = {k: [] for k in "kvsx"}
    data = {k: bytearray() for k in "kvsx"}
    bases = {k: [0] for k in "nkvsx"}
    st = []
    for blk in blocks:
        status, kvs = decode_block(blk, synthetic_seq_num)
        st.append(status)
        base = {k: len(data[k]) for k in "kvsx"}
        for start, end, tr, suffix, value, s, j in kvs:
            for k, x in zip("kvsx", (start, end, suffix, value)):
                offs[k].append(len(data[k]) - base[k])
                data[k] += x
            t.append(tr)
            eo.append(j)
            sp.append(s)
        for k in "kvsx":
            offs[k].append(len(data[k]) - base[k])
            bases[k].append(len(data[k]))
        bases["n"].append(len(t))
    u8 = lambda b: np.frombuffer(bytes(b), np.uint8).copy()  # noqa: E731
    mask = 0
    for s in st:
        mask |= (1 << s) if s else 0
    r = {"trailer": np.array(t, np.uint64), "kv_flags": np.zeros(len(t), np.uint8), "entry_off": np.array(eo, np.uint32),
         "key_off": np.array(offs["k"], np.uint32), "val_off": np.array(offs["v"], np.uint32),
         "key_bytes": u8(data["k"]), "val_bytes": u8(data["v"]), "restarts": None,
         "blk_kv_base": np.array(bases["n"], np.uint64), "blk_key_base": np.array(bases["k"], np.uint64),
         "blk_val_base": np.array(bases["v"], np.uint64), "blk_rst_base": np.zeros(nb + 1, np.uint64),
         "blk_status": np.array(st, np.uint32), "n_kv": len(t), "key_bytes_total": len(data["k"]),
         "val_bytes_total": len(data["v"]), "n_restarts": 0, "status_mask": mask,
         "n_bad_blocks": sum(1 for s in st if s), "n_slow_blocks": 0}
    if extras:
        r.update(span=np.array(sp, np.uint32), suffix_off=np.array(offs["s"], np.uint32),
                 value_off=np.array(offs["x"], np.uint32), suffix_bytes=u8(data["s"]), value_bytes=u8(data["x"]),
                 blk_suffix_base=np.array(bases["s"], np.uint64), blk_value_base=np.array(bases["x"], np.uint64))
    return r


def assert_same(a, b, ctx="", extras=True):
    """Two results in to_host()'s layout: every array and total, exactly."""
    for k in ARRAYS + (EXTRA_KEYS if extras else ()):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k, x[:8], y[:8])
    for k in TOTALS:
        assert int(a[k]) == int(b[k]), (ctx, k, a[k], b[k])


def assert_same_sizes(a, b, ctx=""):
    """The sizes of two results: bases, statuses and totals (what a device result
    with PBL_OVERFLOW holds; its per-KV arrays are unwritten memory)."""
    for k in ("blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status", "blk_suffix_base",
              "blk_value_base"):
        assert np.asarray(a[k]).astype(np.uint64).tolist() == np.asarray(b[k]).astype(np.uint64).tolist(), (ctx, k)
    for k in TOTALS:
        assert int(a[k]) == int(b[k]), (ctx, k, a[k], b[k])


def sized(r) -> dict:
    """What a result with PBL_OVERFLOW holds: the sizes and no bytes."""
    out = dict(r)
    for k in ("trailer", "kv_flags", "entry_off", "key_off", "val_off", "key_bytes", "val_bytes", "span", "suffix_off",
              "value_off", "suffix_bytes", "value_bytes"):
        if k in out and out[k] is not None:
            out[k] = np.zeros(0, np.asarray(out[k]).dtype)
    out["status_mask"] = r["status_mask"] | 1 << N.PBL_OVERFLOW
    return out


# ---- generated blocks -----------------------------------------------------------------------------
def block_of_spans(spans, force=None) -> bytes:
    """spans: [(start, end, [(trailer, suffix, value)])], through the Writer."""
    w = Writer(force)
    for s, e, keys in spans:
        w.add_span(s, e, keys)
    return w.finish()


def rangedel_spans(kvs):
    """A run's KVs [(start, trailer, end)] (fragmented, in order) as Writer spans."""
    spans = []
    for s, t, e in kvs:
        if spans and spans[-1][0] == s and spans[-1][1] == e:
            spans[-1][2].append((t, b"", b""))
        else:
            spans.append((s, e, [(t, b"", b"")]))
    return spans


def random_spans(rng, n_spans, max_keys=3, keylen=(1, 12), gaps=True, range_keys=True, seq_hi=1 << 20):
    """Random fragmented spans over ascending random keys; with `gaps` some
    neighbours do not abut; with `range_keys` suffixes and values are set."""
    keys = set()
    while len(keys) < 2 * n_spans + 2:
        keys.add(bytes(rng.randrange(97, 123) for _ in range(rng.randrange(keylen[0], keylen[1] + 1))))
    keys = sorted(keys)
    spans, i = [], 0
    for _ in range(n_spans):
        ks = []
        for _ in range(rng.randrange(1, max_keys + 1)):
            if range_keys and rng.random() < 0.6:
                ks.append((rng.randrange(1, seq_hi) << 8 | rng.choice((19, 20, 21)),
                           b"@%d" % rng.randrange(100) if rng.random() < 0.7 else b"",
                           bytes(rng.randrange(256) for _ in range(rng.randrange(0, 20)))))
            else:
                ks.append((rng.randrange(1, seq_hi) << 8 | RANGEDEL, b"", b""))
        ks.sort(key=lambda k: -k[0])
        spans.append((keys[i], keys[i + 1], ks))
        i += 2 if gaps and rng.random() < 0.3 else 1
    return spans


def break_block(rng, blk: bytes) -> bytes:
    """A random breakage: a cut, or a flipped byte."""
    b = bytearray(blk)
    if rng.random() < 0.4:
        return bytes(b[: rng.randrange(0, len(b))])
    for _ in range(rng.randrange(1, 3)):
        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


def gap_blocks():
    """(name, block, status): raw column contents that AddSpan never writes."""
    k = [b"a", b"b", b"c", b"d", b"e"]
    t = lambda n: [(9 - i) << 8 | RANGEDEL for i in range(n)]  # noqa: E731
    e = lambda n: [b""] * n  # noqa: E731
    return [
        ("gap in the middle", encode_block(k[:4], [0, 1, 1, 3], t(3), e(3), e(3)), 0),
        ("gap first", encode_block(k[:3], [2, 2, 4], t(4), e(4), e(4)), 0),
        ("rows past the last boundary", encode_block(k[:2], [1, 2], t(5), e(5), e(5)), 0),
        ("gap last", encode_block(k[:3], [0, 2, 2], t(2), e(2), e(2)), BOUNDS),
        ("two gaps in a row", encode_block(k[:5], [0, 1, 1, 1, 2], t(2), e(2), e(2)), BOUNDS),
        ("all gaps", encode_block(k[:3], [1, 1, 1], t(2), e(2), e(2)), BOUNDS),
        ("decreasing idx", encode_block(k[:4], [0, 2, 1, 3], t(3), e(3), e(3)), BOUNDS),
        ("idx past the rows", encode_block(k[:3], [0, 1, 4], t(3), e(3), e(3)), BOUNDS),
        ("one boundary", encode_block(k[:1], [0], t(2), e(2), e(2)), 0),
        ("no boundary", encode_block([], [], t(2), e(2), e(2)), 0),
        # offsets that DecodeColumn does not look at (it bounds a column's last offset only)
        ("suffix past its column", encode_block(k[:2], [0, 1], t(2), [b"x", b""], e(2), offsets={3: [0, 200, 1]}), BOUNDS),
        ("value past its column", encode_block(k[:2], [0, 1], t(2), e(2), [b"x", b""], offsets={4: [0, 200, 1]}), BOUNDS),
        ("suffix far past its column", encode_block(k[:2], [0, 1], t(2), [b"x", b""], e(2), {3: (4, False)},
                                                    {3: [0, 1 << 31, 1]}), BOUNDS),
        ("decreasing boundary offset", encode_block([b"aa", b"b", b"cc"], [0, 1, 2], t(2), e(2), e(2),
                                                    offsets={0: [0, 3, 2, 5]}), BOUNDS),
        ("decreasing suffix offset", encode_block(k[:2], [0, 3], t(3), [b"ab", b"c", b"d"], e(3),
                                                  offsets={3: [0, 3, 2, 4]}), BOUNDS),
        ("decreasing value offset", encode_block(k[:3], [0, 1, 3], t(3), e(3), [b"ab", b"c", b"d"],
                                                 offsets={4: [0, 3, 2, 4]}), BOUNDS),
        ("decreasing suffix offset in rows that are not output", encode_block(k[:2], [0, 1], t(3), [b"a", b"b", b""], e(3),
                                                                              offsets={3: [0, 1, 3, 2]}), 0),
    ]


# ---- a golden columnar table with range deletions -----------------------------------------------------
def _uvarint(x: int) -> bytes:
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def kv_block(rows) -> bytes:
    """colblk.KeyValueBlockWriter (key_value_block.go:30-66): two RawBytes columns."""
    from pebble_amd.keyspan import _put_rawbytes
    buf = bytearray(bytes([1]) + (2).to_bytes(2, "little") + len(rows).to_bytes(4, "little"))
    hdr = len(buf)
    buf += bytes(10)
    for c in range(2):
        buf[hdr + 5 * c] = 3
        buf[hdr + 5 * c + 1: hdr + 5 * c + 5] = len(buf).to_bytes(4, "little")
        _put_rawbytes(buf, [r[c] for r in rows])
    buf.append(0)
    return bytes(buf)


def with_range_dels(data: bytes, spans, block: bytes = None) -> bytes:
    """`data`, a columnar (Pebblev6+) table, re-emitted with an appended keyspan
    block of `spans` (or `block` as it is) plus its 5-byte trailer (no
    compression, the footer's checksum type), a new colblk key-value metaindex
    (the old entries plus rocksdb.range_del2) and a new footer."""
    import oracle
    f = oracle.parse_footer(data[-61:], len(data))
    assert f is not None and f["table_format"] >= N.PBL_TABLE_PEBBLEV6
    ck = f["checksum_type"]
    st, rows = oracle.kv_block_col(oracle.table_block(data, f["metaindex"], ck))
    assert st == 0 and b"rocksdb.range_del2" not in dict(rows)
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
    entries[b"rocksdb.range_del2"] = _uvarint(h[0]) + _uvarint(h[1])
    mh = put(kv_block(sorted(entries.items())))
    ih = f["index"]
    foot = bytearray(flen)
    foot[0] = old[0]
    hs = _uvarint(mh[0]) + _uvarint(mh[1]) + _uvarint(ih[0]) + _uvarint(ih[1])
    foot[1:1 + len(hs)] = hs
    co = flen - 16  # the footer checksum, before version and magic; Pebblev7's attributes before it
    keep = co - 4 if f["table_format"] >= N.PBL_TABLE_PEBBLEV7 else co
    foot[keep:] = old[keep:]
    c = oracle.lib().orc_crc32c_update(0, bytes(foot[:co]), co)
    rest = bytes(foot[co + 4:])
    c = oracle.lib().orc_crc32c_update(c, rest, len(rest))
    foot[co:co + 4] = (((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(body + foot)
