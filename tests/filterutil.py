"""The table bloom filter in plain Python, written from the format (the RocksDB
full-file filter that sstable/tablefilters/bloom reads and writes): the third
statement next to the library's host form and its kernel, which share
filter_core.hip.h.  Nothing here calls the library."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M32 = 0xFFFFFFFF
D, T, C = 0, 1, 2  # PBL_CMP_DEFAULT / TESTKEYS / CRDB
OK, CORRUPT = 0, 15  # PBL_OK / PBL_CORRUPT_FILTER
MAY, BAD = 1, 2
PROBES = [0, 1, 1, 2, 3, 3, 4, 4, 5, 5, 6]


def load_golden():
    with open(os.path.join(GOLDEN, "filter.json")) as f:
        return json.load(f)


def _sext(b):
    return (b - 256 if b >= 128 else b) & M32


def bloom_hash(b: bytes) -> int:
    m = 0xC6A4A793
    h = 0xBC9F1D34 ^ ((len(b) * m) & M32)
    full = len(b) & ~3
    for i in range(0, full, 4):
        h = (h + int.from_bytes(b[i:i + 4], "little")) & M32
        h = (h * m) & M32
        h ^= h >> 16
    t = b[full:]
    if t:
        for j in range(len(t) - 1, -1, -1):
            h = (h + ((_sext(t[j]) << (8 * j)) & M32)) & M32
        h = (h * m) & M32
        h ^= h >> 24
    return h


def split(comparer: int, key: bytes) -> int:
    if comparer == T:
        i = key.rfind(b"@")
        return i if i >= 0 else len(key)
    if comparer == C:
        if not key:
            return 0
        return len(key) - key[-1] if key[-1] <= len(key) else 0
    return len(key)


def prefix_hash(comparer: int, key: bytes) -> int:
    return bloom_hash(key[:split(comparer, key)])


def parse(f: bytes):
    """(n_lines, n_probes, status); n_lines == 0 for an empty or corrupt filter."""
    if len(f) <= 5:
        return 0, 0, OK
    n = len(f) - 5
    n_lines = int.from_bytes(f[n + 1:n + 5], "little")
    if n_lines == 0 or n // n_lines != 64:
        return 0, f[n], CORRUPT
    return n_lines, f[n], OK


def may_bits(f: bytes, h: int) -> int:
    """The `may` byte of hash h in filter f."""
    n_lines, n_probes, st = parse(f)
    if st != OK:
        return MAY | BAD
    if n_lines == 0:
        return 0
    delta = (h >> 17 | h << 15) & M32
    line = (h % n_lines) * 64
    for _ in range(n_probes):
        if not f[line + ((h >> 3) & 63)] & (1 << (h & 7)):
            return 0
        h = (h + delta) & M32
    return MAY


def build(keys, comparer: int, bits_per_key: int) -> bytes:
    hs = []
    for k in keys:
        h = prefix_hash(comparer, k)
        if not hs or hs[-1] != h:
            hs.append(h)
    if not hs:
        return b""
    n_lines = ((len(hs) * bits_per_key + 511) // 512) | 1
    n_probes = PROBES[min(bits_per_key, 10)]
    f = bytearray(n_lines * 64 + 5)
    for h in hs:
        delta = (h >> 17 | h << 15) & M32
        line = (h % n_lines) * 64
        for _ in range(n_probes):
            f[line + ((h >> 3) & 63)] |= 1 << (h & 7)
            h = (h + delta) & M32
    f[n_lines * 64] = n_probes
    f[n_lines * 64 + 1:] = n_lines.to_bytes(4, "little")
    return bytes(f)


def with_trailer(f: bytes, n_probes=None, n_lines=None) -> bytes:
    """f with its trailer's fields replaced."""
    b = bytearray(f)
    if n_probes is not None:
        b[-5] = n_probes
    if n_lines is not None:
        b[-4:] = n_lines.to_bytes(4, "little")
    return bytes(b)


def edge_keys():
    """Keys of every length 0 .. 40 from the bytes 0x00, 0x7f, 0x80, 0xff, so
    that every tail length meets a sign-extended byte."""
    pat = bytes([0x00, 0x7F, 0x80, 0xFF])
    out = []
    for n in range(41):
        for r in range(4):
            out.append(bytes(pat[(i + r) & 3] for i in range(n)))
        out.append(bytes([0x80 + (i * 37 & 0x7F) for i in range(n)]))
    return out


def member_keys(n: int, tag: bytes = b"k"):
    return [tag + b"%06d" % (i * 7) for i in range(n)]


def filter_cases():
    """(name, filter bytes, member keys): 1, 3 and 35 lines at 1, 5, 10 and 20
    bits per key, the trailer edge cases, the empty and the corrupt ones."""
    out = []
    for bpk in (1, 5, 10, 20):
        for lines in (1, 3, 35):
            n = max(1, ((lines - 1) * 512 + 256) // bpk) if lines > 1 else max(1, 300 // bpk)
            keys = member_keys(n, b"m%d_%d_" % (bpk, lines))
            f = build(keys, D, bpk)
            assert parse(f)[0] == lines, (bpk, lines, parse(f))
            out.append((f"bpk{bpk}_lines{lines}", f, keys))
    keys = member_keys(100, b"t")
    f = build(keys, D, 10)
    out.append(("probes0", with_trailer(f, n_probes=0), keys))
    f30 = bytearray(build(keys, D, 10))
    f30[:-5] = b"\xff" * (len(f30) - 5)
    f30[7] = 0xFE  # one clear bit that 30 probes may meet
    out.append(("probes30", with_trailer(bytes(f30), n_probes=30), keys))
    out.append(("probes255", with_trailer(bytes(f30), n_probes=255), keys))
    out.append(("len0", b"", keys))
    out.append(("len5", b"\x06\x01\x00\x00\x00", keys))
    out.append(("lines0", with_trailer(f, n_lines=0), keys))
    out.append(("lines_mismatch", with_trailer(f, n_lines=parse(f)[0] + 2), keys))
    out.append(("lines_huge", with_trailer(f, n_lines=0xFFFFFFFF), keys))
    out.append(("short_body", f[64:], keys))
    return out


def probe_keys(members, n_other=60):
    return list(members[:60]) + [b"zz%05d" % i for i in range(n_other)]


def expected_probe(filters, keys, comparer, which=None):
    """(may, hash, status) as pbl_filter_probe defines them."""
    hs = [prefix_hash(comparer, k) for k in keys]
    st = [parse(f)[2] for f in filters]
    if which is None:
        may = [may_bits(f, h) for f in filters for h in hs]
    else:
        may = [may_bits(filters[w], h) if w < len(filters) else MAY | BAD for w, h in zip(which, hs)]
    return may, hs, st


# ---- a row-format table with a bloom filter, for tests that need more than the reference's ------------
def _uvarint(x: int) -> bytes:
    out = bytearray()
    while x >= 0x80:
        out.append(x & 0x7F | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def bloom_table(template: bytes, keys, bits_per_key: int = 10, per_block: int = 50) -> bytes:
    """A table in `template`'s format (a Pebblev1 row table: its properties block
    and footer layout are reused) holding `keys` (sorted, bytewise comparer) as
    SET KVs in row data blocks, a one-level row index, the filter block
    tests/filterutil.build writes for them, and a metaindex naming the filter
    and the properties."""
    import oracle
    from pebble_amd.rowblk import Writer, make_trailer
    f = oracle.parse_footer(template[-61:], len(template))
    assert f is not None and f["table_format"] == 3 and f["footer"][1] == 53
    ck = f["checksum_type"]
    st, rows, _ = oracle.rowblk_decode_block(oracle.table_block(template, f["metaindex"], ck), 0x4)
    assert st == 0
    props = oracle.table_block(template, oracle.decode_handle(dict((r[0], r[2]) for r in rows)[b"rocksdb.properties"], 0)[0], ck)
    body = bytearray()

    def put(block):
        off = len(body)
        body.extend(block + b"\0")
        body.extend(oracle.block_checksum(ck, block + b"\0").to_bytes(4, "little"))
        return _uvarint(off) + _uvarint(len(block))

    index = Writer(1)
    for i in range(0, len(keys), per_block):
        w = Writer(16)
        for j, k in enumerate(keys[i:i + per_block]):
            w.add(k, make_trailer(i + j + 1, 1), b"v%d" % (i + j))
        last = keys[min(i + per_block, len(keys)) - 1]
        index.add(last, make_trailer((1 << 56) - 1, 17), put(w.finish()))  # a separator key (SeqNumMax, kind 17)
    ih = put(index.finish())
    meta = Writer(1)
    meta.add_raw(b"fullfilter.rocksdb.BuiltinBloomFilter", put(build(keys, D, bits_per_key)))
    meta.add_raw(b"rocksdb.properties", put(props))
    mh = put(meta.finish())
    old = template[f["footer"][0]: f["footer"][0] + 53]
    foot = bytearray(old)
    foot[1:41] = (mh + ih).ljust(40, b"\0")
    return bytes(body) + bytes(foot)
