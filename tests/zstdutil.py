"""Zstandard frames for the zstd decoder's tests (RFC 8878), in pure Python:

  * census(): a header walker that decodes nothing and counts the format
    features present in a run of frames, so a test can state which features
    its corpus holds instead of assuming them;
  * low-entropy corpora whose literals facebook/zstd Huffman-codes;
  * frame(): an assembler that writes frames from explicit parts, for what
    the library never emits on request (direct Huffman weights, RLE literals,
    RLE tables, forced size formats, the 3-byte sequence count, repeat-offset
    code 3, header variants);
  * route wrappers that send one frame down each of the device's three routes;
  * zstd_gpu_corpus(): the corpus of tests/test_zstd_forms_gpu.py, whose
    census tests/test_zstd_forms.py holds to a coverage floor on the CPU.

The ground truth for every assembled frame is facebook/zstd itself (the codec
pyarrow bundles): libzstd()."""
import collections
import functools
import heapq
import random

MAGIC = 0xFD2FB528
LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
           1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
DEFAULTS = ((LL_DEF, 6), (OF_DEF, 5), (ML_DEF, 6))   # LL, OF, ML: the order of the modes byte
MAX_AL = (9, 8, 9)
MODES = ("predefined", "rle", "fse", "repeat")
LTYPES = ("raw", "rle", "huffman", "treeless")
TABLES = ("ll", "of", "ml")


def uvarint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append(n & 0x7F | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def libzstd(frame: bytes, n: int) -> bytes:
    """facebook/zstd's decoding of `frame` (n decoded bytes); raises on a frame it rejects."""
    import pyarrow as pa
    return pa.Codec("zstd").decompress(frame, decompressed_size=n, asbytes=True)


def compress(data: bytes, level: int, checksum: bool = False) -> bytes:
    """A frame written by facebook/zstd.  The codec has no checksum switch, so
    checksum=True sets the frame header's flag and appends the low 32 bits of
    XXH64(content), which is all the library's own switch does."""
    import pyarrow as pa
    f = pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)
    return add_checksum(f, data) if checksum else f


def add_checksum(frame: bytes, content: bytes) -> bytes:
    import xxhash
    f = bytearray(frame)
    assert int.from_bytes(f[:4], "little") == MAGIC and not f[4] & 4
    f[4] |= 4
    return bytes(f) + (xxhash.xxh64(content).intdigest() & 0xFFFFFFFF).to_bytes(4, "little")


# ---- the header walker ------------------------------------------------------------
def _ncount_len(b: bytes, at: int) -> int:
    """Bytes of the FSE table description at b[at:] (FSE_readNCount's walk)."""
    def fwd(bit, k):
        return (int.from_bytes(b[at + (bit >> 3): at + (bit >> 3) + 4], "little") >> (bit & 7)) & ((1 << k) - 1)
    al = fwd(0, 4) + 5
    bit, remaining, threshold, nbits = 4, (1 << al) + 1, 1 << al, al + 1
    while remaining > 1:
        mx = 2 * threshold - 1 - remaining
        low = fwd(bit, nbits - 1)
        if low < mx:
            v, bit = low, bit + nbits - 1
        else:
            v, bit = fwd(bit, nbits), bit + nbits
            if v >= threshold:
                v -= mx
        remaining -= abs(v - 1)
        if v == 1:
            while True:
                r, bit = fwd(bit, 2), bit + 2
                if r != 3:
                    break
        while remaining < threshold and nbits > 1:
            nbits, threshold = nbits - 1, threshold >> 1
    return (bit + 7) // 8


def walk(data: bytes):
    """The frames of `data` as dicts of header fields and byte ranges (offsets
    into `data`); nothing is decoded.  `data` must be well formed."""
    frames, q = [], 0
    while q < len(data):
        magic = int.from_bytes(data[q:q + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            sz = int.from_bytes(data[q + 4:q + 8], "little")
            frames.append({"skippable": True, "at": q, "end": q + 8 + sz})
            q += 8 + sz
            continue
        assert magic == MAGIC, hex(magic)
        fhd = data[q + 4]
        f = {"skippable": False, "at": q, "single": bool(fhd & 0x20), "checksum": bool(fhd & 4),
             "did_bytes": (0, 1, 2, 4)[fhd & 3], "blocks": []}
        f["fcs_bytes"] = ((1 if f["single"] else 0), 2, 4, 8)[fhd >> 6]
        q += 5 + (0 if f["single"] else 1)
        f["dict_id"] = int.from_bytes(data[q:q + f["did_bytes"]], "little")
        q += f["did_bytes"] + f["fcs_bytes"]
        while True:
            bh = int.from_bytes(data[q:q + 3], "little")
            blk = {"type": ("raw", "rle", "compressed")[(bh >> 1) & 3], "at": q + 3, "size": bh >> 3}
            q += 3
            if blk["type"] == "compressed":
                _walk_block(data, q, blk)
            q += 1 if blk["type"] == "rle" else blk["size"]
            f["blocks"].append(blk)
            if bh & 1:
                break
        q += 4 if f["checksum"] else 0
        f["end"] = q
        frames.append(f)
    assert q == len(data)
    return frames


def _walk_block(d: bytes, q: int, blk: dict):
    end = q + blk["size"]
    b0 = d[q]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    blk["ltype"], blk["sf"] = LTYPES[lt], 0 if lt < 2 and sf == 2 else sf   # (raw / RLE: 0 and 2 are the one 1-byte form)
    if lt < 2:
        h = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = int.from_bytes(d[q:q + h], "little") >> (3 if h == 1 else 4)
        q += h + (regen if lt == 0 else 1)
    else:
        h = 3 if sf < 2 else 4 if sf == 2 else 5
        v = int.from_bytes(d[q:q + h], "little")
        nb = 10 if sf < 2 else 14 if sf == 2 else 18
        regen, csize = (v >> 4) & ((1 << nb) - 1), v >> (4 + nb)
        blk["streams"] = 1 if sf == 0 else 4
        c = q + h
        if lt == 2:
            hb = d[c]
            blk["weights"] = "direct" if hb >= 128 else "fse"
            t = 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)
            blk["huf_desc"] = (c, c + t)
            c += t
        blk["huf_streams"] = (c, q + h + csize)
        q += h + csize
    blk["regen"] = regen
    n = d[q]
    if n < 128:
        blk["nseq_bytes"], q = (1 if n else 0), q + 1
    elif n < 255:
        n, blk["nseq_bytes"], q = ((n - 128) << 8) + d[q + 1], 2, q + 2
    else:
        n, blk["nseq_bytes"], q = d[q + 1] + (d[q + 2] << 8) + 0x7F00, 3, q + 3
    blk["nseq"] = n
    if n:
        modes = d[q]
        blk["modes"] = (modes >> 6, (modes >> 4) & 3, (modes >> 2) & 3)
        t0 = q = q + 1
        for m in blk["modes"]:
            q += 1 if m == 1 else _ncount_len(d, q) if m == 2 else 0
        blk["tables"], blk["seq_bits"] = (t0, q), (q, end)
    assert q <= end


def census(frames: bytes) -> collections.Counter:
    """How often each format feature occurs in a run of frames."""
    c = collections.Counter()
    for f in walk(frames):
        if f["skippable"]:
            c["skippable"] += 1
            continue
        c["frame"] += 1
        c["single_segment" if f["single"] else "window_descriptor"] += 1
        c["fcs_bytes_%d" % f["fcs_bytes"]] += 1
        c["dict_id_bytes_%d" % f["did_bytes"]] += 1
        if f["checksum"]:
            c["checksum"] += 1
        c["frame_multi_block" if len(f["blocks"]) > 1 else "frame_single_block"] += 1
        for b in f["blocks"]:
            c["block_" + b["type"]] += 1
            if b["type"] != "compressed":
                continue
            c["lit_" + b["ltype"]] += 1
            c["lit_%s_sf%d" % (b["ltype"], b["sf"])] += 1
            if "streams" in b:
                c["huf_streams_%d" % b["streams"]] += 1
            if "weights" in b:
                c["huf_weights_" + b["weights"]] += 1
            c["nseq_0" if not b["nseq"] else "nseq_%dbyte" % b["nseq_bytes"]] += 1
            for t, m in zip(TABLES, b.get("modes", ())):
                c["%s_%s" % (t, MODES[m])] += 1
    return c


def first_block_nseq(frames: bytes):
    """The sequence count of each frame's first block (0 for a raw or RLE block)."""
    return [f["blocks"][0].get("nseq", 0) for f in walk(frames) if not f["skippable"]]


# ---- low-entropy corpora ------------------------------------------------------------
def corpus(rng, kind, n):
    """n bytes: 0 random, 1 letters-only words, 2 one byte repeated, 3 words with a few random bytes between them."""
    words = [bytes(rng.choice(b"abcdefghij") for _ in range(rng.randint(2, 9))) for _ in range(300)]
    if kind == 0:
        return rng.randbytes(n)
    if kind == 1:
        return b" ".join(rng.choice(words) for _ in range(n // 5 + 1))[:n]
    if kind == 2:
        return bytes([rng.choice(b"ab")]) * n
    return b"".join(rng.choice(words) + rng.randbytes(rng.randint(0, 3)) for _ in range(n // 6 + 1))[:n]


def letters(rng, n, mixed=False):
    """corpus kind 1 (letters-only words), or kind 3 (a few random bytes between them)."""
    return corpus(rng, 3 if mixed else 1, n)


def few_symbols(rng, n):
    return bytes(rng.choice(b"ab") if rng.random() < 0.9 else rng.choice(b"cdefg") for _ in range(n))


def zero_one(rng, n):
    return bytes(rng.choice(b"01") for _ in range(n))


def low_entropy(rng, i, n):
    return (letters(rng, n), few_symbols(rng, n), letters(rng, n, True), zero_one(rng, n))[i % 4]


# ---- bit writers ------------------------------------------------------------------------
class BitW:
    """Bits appended from bit 0 up; bytes() adds the backward stream's end mark."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def add(self, v, k):
        assert 0 <= v < (1 << k) or (k == 0 and v == 0), (v, k)
        self.acc |= v << self.n
        self.n += k
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def bytes(self, mark=True):
        if mark:
            self.add(1, 1)
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- FSE ----------------------------------------------------------------------------------
def fse_table(norm, al):
    """The decoding table [(symbol, bits, base)] of normalised counts (RFC 8878 §4.1.1)."""
    size = 1 << al
    sym_of, nxt, high = [0] * size, {}, size - 1
    for s, p in enumerate(norm):
        if p == -1:
            sym_of[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = p
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym_of[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    T = []
    for u in range(size):
        s = sym_of[u]
        x = nxt[s]
        nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        T.append((s, nb, (x << nb) - size))
    return T


class FseEnc:
    """Encodes against a decoding table by searching it: the state before
    `nxt` for symbol s is the one whose [base, base + 2^bits) holds nxt."""

    def __init__(self, T, al):
        self.T, self.al, self.by_sym = T, al, collections.defaultdict(list)
        for u, (s, nb, base) in enumerate(T):
            self.by_sym[s].append((base, nb, u))

    def state(self, sym, nxt=None):
        st = self.by_sym[sym]
        assert st, "symbol %d is not in the table" % sym
        if nxt is None:
            return st[0][2], 0, 0
        for base, nb, u in st:
            if base <= nxt < base + (1 << nb):
                return u, nxt - base, nb
        raise AssertionError("no state")


def rle_enc(sym):
    """An RLE table: one state, no bits."""
    return FseEnc([(sym, 0, 0)], 0)


def normalize(hist, al):
    """Counts -> normalised counts summing to 2^al, every present symbol >= 1."""
    size, total = 1 << al, sum(hist.values())
    assert 2 <= len(hist) <= size
    norm = {s: max(1, c * size // total) for s, c in hist.items()}
    diff = size - sum(norm.values())
    while diff:
        s = max(norm, key=lambda k: norm[k])
        step = diff if diff > 0 else max(diff, 1 - norm[s])
        assert step
        norm[s] += step
        diff -= step
    return [norm.get(s, 0) for s in range(max(norm) + 1)]


def ncount(norm, al) -> bytes:
    """The table description FSE_readNCount reads (RFC 8878 §4.1.1)."""
    w = BitW()
    w.add(al - 5, 4)
    remaining, threshold, nbits, s = (1 << al) + 1, 1 << al, al + 1, 0
    while remaining > 1:
        p = norm[s]
        mx, v = 2 * threshold - 1 - remaining, p + 1
        if v < mx:
            w.add(v, nbits - 1)
        else:
            w.add(v if v < threshold else v + mx, nbits)
        remaining -= abs(p)
        s += 1
        if p == 0:
            z = 0
            while norm[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.add(3, 2)
                z -= 3
            w.add(z, 2)
        while remaining < threshold and nbits > 1:
            nbits, threshold = nbits - 1, threshold >> 1
    assert s == len(norm)
    return w.bytes(mark=False)


# ---- Huffman --------------------------------------------------------------------------------
def huf_lengths(lits: bytes, limit=11):
    """Code lengths of a complete prefix code over the symbols of `lits`, none past `limit`."""
    hist = collections.Counter(lits)
    assert len(hist) >= 2, "Huffman literals need two distinct symbols"
    while True:
        heap = [(c, s, (s,)) for s, c in hist.items()]
        heapq.heapify(heap)
        ln = dict.fromkeys(hist, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                ln[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(ln.values()) <= limit:
            return ln
        hist = collections.Counter({s: (c + 1) // 2 for s, c in hist.items()})  # flatten and retry


def huf_weights(ln):
    """Code lengths -> the weights of symbols 0..max (0: absent)."""
    log = max(ln.values())
    return [log + 1 - ln[s] if s in ln else 0 for s in range(max(ln) + 1)]


def huf_codes(w):
    """{symbol: (code, bits)} of weights in HUF_readDTableX1's order: weight 1
    first, symbols in order within a weight."""
    total = sum(1 << (k - 1) for k in w if k)
    log = total.bit_length() - 1
    assert total == 1 << log, "the weights must fill a power of two"
    start, acc = {}, 0
    for k in range(1, log + 1):
        start[k] = acc
        acc += w.count(k) << (k - 1)
    codes = {}
    for s, k in enumerate(w):
        if k:
            codes[s] = (start[k] >> (k - 1), log + 1 - k)
            start[k] += 1 << (k - 1)
    return codes


def huf_stream(lits: bytes, codes) -> bytes:
    w = BitW()
    for s in reversed(lits):
        w.add(*codes[s])
    return w.bytes()


def direct_weights(w) -> bytes:
    """The nibble form of a tree description: every weight but the last symbol's."""
    w = w[:-1]
    assert 1 <= len(w) <= 128, "the direct form holds at most 128 weights"
    nib = w + [0] * (len(w) & 1)
    return bytes([127 + len(w)]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))


# ---- blocks -------------------------------------------------------------------------------------
class State:
    """What a frame's later blocks may repeat, and the executor's history."""

    def __init__(self):
        self.codes, self.enc, self.rep, self.out, self.valid = None, [None, None, None], [1, 4, 8], bytearray(), True


def execute(st: State, lits: bytes, seqs):
    """The sequences' intended output, appended to st.out (RFC 8878 §3.1.1.4-5).
    An offset of 0 or past the output marks the frame invalid."""
    out, rep, lp = st.out, st.rep, 0
    for ll, ml, off in seqs:
        out += lits[lp:lp + ll]
        lp += ll
        if off > 0:
            rep[:] = [off, rep[0], rep[1]]
        else:
            k = -off - 1 + (ll == 0)
            if k:
                o = rep[0] - 1 if k == 3 else rep[k]
                rep[:] = [o, rep[0], rep[2] if k == 1 else rep[1]]
        o = rep[0]
        if not 0 < o <= len(out):
            st.valid = False
            out += bytes(ml)
            continue
        for _ in range(ml):
            out.append(out[-o])
    out += lits[lp:]


def _code(v, base):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c


def literals_section(st: State, lits: bytes, ltype="raw", sf=None, empty_last_stream=False, weights=None) -> bytes:
    n = len(lits)
    if ltype in ("raw", "rle"):
        if sf is None:
            sf = 0 if n < 32 else 1 if n < 4096 else 3
        assert n < (32, 4096, 32, 1 << 20)[sf]
        t = LTYPES.index(ltype)   # (the 1-byte form has a 1-bit size format: bit 3 is the size's lowest bit)
        h = bytes([n << 3 | t]) if sf in (0, 2) else (n << 4 | sf << 2 | t).to_bytes(2 if sf == 1 else 3, "little")
        if ltype == "rle":
            assert n and lits == lits[:1] * n
        return h + (lits if ltype == "raw" else lits[:1])
    desc = b""
    if ltype == "huffman":
        w = weights or huf_weights(huf_lengths(lits))
        st.codes = huf_codes(w)
        desc = direct_weights(w)
    assert st.codes is not None
    if sf == 0 or (sf is None and n < 6):
        sf, body = 0, huf_stream(lits, st.codes)
    else:
        seg = (n + 3) // 4
        assert n >= 6
        parts = [huf_stream(lits[i * seg:(i + 1) * seg], st.codes) for i in range(4)]
        if empty_last_stream:
            assert 3 * seg == n
            parts[3] = b""
        body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
        if sf is None:
            m = max(n, len(desc) + len(body))
            sf = 1 if m < 1024 else 2 if m < 16384 else 3
    nb = 10 if sf < 2 else 14 if sf == 2 else 18
    csize = len(desc) + len(body)
    assert n < 1 << nb and csize < 1 << nb, (n, csize, sf)
    h = (LTYPES.index(ltype) | sf << 2 | n << 4 | csize << (4 + nb)).to_bytes(3 if sf < 2 else 4 if sf == 2 else 5, "little")
    return h + desc + body


def sequences_section(st: State, seqs, modes=("predefined",) * 3, al=(None,) * 3, nseq_bytes=None) -> bytes:
    n = len(seqs)
    if n == 0:
        return b"\x00"
    if nseq_bytes is None:
        nseq_bytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if nseq_bytes == 1:
        assert n < 128
        out = bytearray([n])
    elif nseq_bytes == 2:
        assert n < 0x7F00
        out = bytearray([128 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n < 0x7F00 + 65536
        out = bytearray([255]) + (n - 0x7F00).to_bytes(2, "little")
    # codes and extra bits: (LL, OF, ML) per sequence
    cs = []
    for ll, ml, off in seqs:
        ofv = off + 3 if off > 0 else -off
        lc, oc, mc = _code(ll, LL_BASE), ofv.bit_length() - 1, _code(ml, ML_BASE)
        cs.append(((lc, oc, mc), ((ll - LL_BASE[lc], LL_BITS[lc]), (ofv - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]))))
    out.append(sum(MODES.index(m) << s for m, s in zip(modes, (6, 4, 2))))
    for t, m in enumerate(modes):
        syms = [c[0][t] for c in cs]
        if m == "predefined":
            st.enc[t] = FseEnc(fse_table(DEFAULTS[t][0], DEFAULTS[t][1]), DEFAULTS[t][1])
        elif m == "rle":
            assert len(set(syms)) == 1, "an RLE table codes one symbol"
            st.enc[t] = rle_enc(syms[0])
            out.append(syms[0])
        elif m == "fse":
            a = al[t] or 6
            assert 5 <= a <= MAX_AL[t]
            norm = normalize(collections.Counter(syms), a)
            st.enc[t] = FseEnc(fse_table(norm, a), a)
            out += ncount(norm, a)
        # "repeat": st.enc[t] as the earlier block left it (None in a first block: the caller builds a corrupt frame)
    enc = [e or FseEnc(fse_table(DEFAULTS[t][0], DEFAULTS[t][1]), DEFAULTS[t][1]) for t, e in enumerate(st.enc)]
    # written backwards: what the decoder reads last goes in first
    w, nxt = BitW(), [None, None, None]
    for i in range(n - 1, -1, -1):
        codes, extra = cs[i]
        s = [enc[t].state(codes[t], nxt[t]) for t in range(3)]
        if i < n - 1:
            for t in (1, 2, 0):   # read LL, ML, OF
                w.add(s[t][1], s[t][2])
        for t in (0, 2, 1):       # read OF, ML, LL
            w.add(*extra[t])
        nxt = [x[0] for x in s]
    for t in (2, 1, 0):           # read LL, OF, ML
        w.add(nxt[t], enc[t].al)
    return bytes(out) + w.bytes()


def frame(blocks, single=True, fcs_bytes=None, checksum=False, did_bytes=0, dict_id=0, bad_checksum=False, invalid=False):
    """A zstd frame from explicit parts; returns (frame, content).

    blocks: a list of
      ("raw", data) | ("rle", byte, n) |
      ("comp", literals, [(ll, ml, offset)], {options})   offset > 0, or -1 / -2 / -3 for a repeat code
    with options ltype ("raw" | "rle" | "huffman" | "treeless"), sf (the
    literals header's size format, forced), empty_last_stream, weights (the
    Huffman weights of symbols 0..max, forced), modes (one of
    "predefined" | "rle" | "fse" | "repeat" for each of LL, OF, ML), al (the
    accuracy log of each FSE-described table), nseq_bytes (1 | 2 | 3), hidden
    (the block is encoded, so later blocks can refer to its tree and tables,
    but left out of the frame and of its content: the repeated tree or table
    is then the frame's one defect).
    Huffman literals carry direct weights; size format 0 is the 1-stream form.
    single=False writes a window descriptor no smaller than the content;
    invalid=True lets the sequences reach before the output (a corrupt frame)."""
    import xxhash
    st, body, biggest = State(), bytearray(), 0
    for i, b in enumerate(blocks):
        last = i == len(blocks) - 1
        if b[0] == "raw":
            st.out += b[1]
            body += (last | 0 << 1 | len(b[1]) << 3).to_bytes(3, "little") + b[1]
        elif b[0] == "rle":
            st.out += bytes([b[1]]) * b[2]
            body += (last | 1 << 1 | b[2] << 3).to_bytes(3, "little") + bytes([b[1]])
        else:
            o = dict(b[3]) if len(b) > 3 else {}
            hidden = o.pop("hidden", False)
            sec = literals_section(st, b[1], o.pop("ltype", "raw"), o.pop("sf", None), o.pop("empty_last_stream", False),
                                   o.pop("weights", None))
            sec += sequences_section(st, b[2], **o)
            if hidden:   # its tree and tables stay in st; its output and repeat offsets never existed
                continue
            execute(st, b[1], b[2])
            assert len(sec) < 1 << 17
            biggest = max(biggest, len(sec))
            body += (last | 2 << 1 | len(sec) << 3).to_bytes(3, "little") + sec
    content = bytes(st.out)
    n = len(content)
    assert st.valid or invalid, "an offset of 0 or past the output"
    # facebook/zstd holds a block to min(window, 128 KiB), and a single-segment frame's window is its content
    assert biggest <= (n if single else max(n, 1024)), "a block larger than the window: use single=False"
    if fcs_bytes is None:
        fcs_bytes = (1 if n < 256 else 2 if n < 65536 + 256 else 4) if single else 0
    assert fcs_bytes in ((1, 2, 4, 8) if single else (0, 2, 4, 8)) and (fcs_bytes != 1 or n < 256)
    assert fcs_bytes != 2 or 256 <= n < 65536 + 256
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6 | single << 5 | checksum << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    hdr = MAGIC.to_bytes(4, "little") + bytes([fhd])
    if not single:
        hdr += bytes([max(0, (max(n, 1) - 1).bit_length() - 10) << 3])
    hdr += dict_id.to_bytes(did_bytes, "little") + (n - 256 if fcs_bytes == 2 else n if fcs_bytes else 0).to_bytes(fcs_bytes, "little")
    tail = b""
    if checksum:
        tail = ((xxhash.xxh64(content).intdigest() ^ bad_checksum) & 0xFFFFFFFF).to_bytes(4, "little")
    return hdr + bytes(body) + tail, content


# ---- route wrappers -------------------------------------------------------------------------------
def skippable(n: int, magic=0x184D2A50) -> bytes:
    return magic.to_bytes(4, "little") + n.to_bytes(4, "little") + bytes(i * 7 & 255 for i in range(n))


def as_is(frame_: bytes, n: int) -> bytes:
    """The Pebble zstd block of the frame alone.  zstd_prep_kernel takes it onto
    the four-kernel batch path when it is one frame of one compressed, last
    block decoding to n <= 36864 bytes with no treeless literals and no repeat
    table (zstd_fast.hip.h:186-247, :324) -- and while the batch's sequence
    area lasts (:375); zstd_kernel takes every other block."""
    return uvarint(n) + frame_


def skippable_prefix(frame_: bytes, n: int) -> bytes:
    """A 5-byte skippable frame first: zstd_prep_kernel's magic check
    (zstd_fast.hip.h:194) leaves the block to zstd_kernel, which decodes it in
    LDS while the compressed bytes, these 13 included, are <= 28672 and
    n <= 36864 (zstd.hip:83); route() tells, and tests/test_zstd_forms.py
    holds the corpus to it."""
    return uvarint(n) + skippable(5, 0x184D2A53) + frame_


def skippable_pad(frame_: bytes, n: int) -> bytes:
    """A skippable frame of more than 28672 bytes first: past zstd.hip:83's LDS
    limit, so zstd_kernel decodes from and to global memory (zstd.hip:111)."""
    return uvarint(n) + skippable(28672 + 1 + n % 13) + frame_


ROUTES = (as_is, skippable_prefix, skippable_pad)
K_IN, K_OUT, SEQ_PER_BLOCK = 28672, 36864, 4096   # kIn, kOut (zstd_dec.hip.h:11-12), kSeqPerBlock (zstd_fast.hip.h:52)


def route(block: bytes) -> str:
    """The route a well-formed Pebble zstd block takes on the device, by the
    conditions the code states: "batch" for one frame with no dictionary-ID
    field that is one compressed, last block of at most kOut decoded bytes
    with no treeless literals and no repeat table (zstd_fast.hip.h:186-247,
    :324; the kHdrWin limits hold for every frame, a tree description being at
    most 129 bytes) -- while the sequence area lasts; otherwise "lds" while
    the compressed bytes are <= kIn and the decoded <= kOut (zstd.hip:83), and
    "global" past either."""
    n = used = 0
    while True:
        n |= (block[used] & 0x7F) << (7 * used)
        used += 1
        if block[used - 1] < 0x80:
            break
    frames = walk(block[used:])
    f = frames[0]
    if len(frames) == 1 and not f["skippable"] and n <= K_OUT and f["did_bytes"] == 0 and len(f["blocks"]) == 1:
        b = f["blocks"][0]
        if b["type"] == "compressed" and b["ltype"] != "treeless" and 3 not in b.get("modes", ()):
            return "batch"
    return "lds" if len(block) - used <= K_IN and n <= K_OUT else "global"


def min_fallbacks(nseq, n_blocks) -> int:
    """How many of a batch's blocks (first-block sequence counts `nseq`, among
    n_blocks blocks of any codec) the batch path must hand to zstd_kernel,
    whatever order its counter serves them in: the area holds n_blocks x
    kSeqPerBlock sequences, a block fits while the counter, which never goes
    back, has room for it (zstd_fast.hip.h:87, :373-375) -- so at most as many
    fit as do smallest first."""
    room, fit = n_blocks * SEQ_PER_BLOCK, 0
    for k in sorted(nseq):
        if k > room:
            break
        room, fit = room - k, fit + 1
    return len(nseq) - fit


# ---- the assembled forms ------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name frame want feature")   # feature: census keys the case was built for


def _text(rng, n, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _skew(rng, n, top):
    """n literals over symbols 0..top, both ends present, skewed so code lengths differ."""
    syms = [0, top] + [min(top, int(rng.expovariate(0.08))) for _ in range(n - 2)]
    rng.shuffle(syms)
    return bytes(syms)


def _seqs_for(rng, n_lits, n_seq, offs=(1, 2, 3, 5, 9, 17), mls=(3, 4, 5, 8, 20), rep_every=0):
    """n_seq sequences over at most n_lits literals whose offsets stay inside the output."""
    seqs, made, left = [], 0, n_lits
    for i in range(n_seq):
        ll = min(left, rng.choice((1, 1, 2, 3, 7, 17)) if i else max(2, min(left, 20)))
        left -= ll
        made += ll
        ml = rng.choice(mls)
        off = min(rng.choice(offs), made)
        if rep_every and i and i % rep_every == 0:
            off = -1
        seqs.append((ll, ml, off))
        made += ml
    return seqs


@functools.lru_cache(maxsize=None)
def assembled_forms():
    """Every assembled frame of the forms tests: (name, frame, content, census
    keys the frame was built to show).  All are valid zstd."""
    rng = random.Random(77)
    out = []

    def add(name, blocks, feature, **hdr):
        f, want = frame(blocks, **hdr)
        out.append(Case(name, f, want, tuple(feature)))

    # direct weights: 1, 2, 3, 127 and 128 weights listed (2 .. 129 with the implied last one)
    for nw in (1, 2, 3, 127, 128):
        lits = _skew(rng, 300 + nw, nw)
        add("direct_weights_%d" % nw, [("comp", lits, _seqs_for(rng, len(lits) - 9, 12), {"ltype": "huffman"})],
            ["huf_weights_direct", "lit_huffman_sf1"])
    # 1 stream (size format 0) and 4 streams at forced size formats 1, 2, 3
    for sf, n in ((0, 5), (0, 700), (0, 1023), (1, 333), (1, 1023), (2, 334), (2, 5000), (3, 335), (3, 17001)):
        lits = _text(rng, n, b"aaaabbbccdeefgh \n")
        add("huffman_sf%d_%d" % (sf, n), [("comp", lits, _seqs_for(rng, n - 3, min(40, n // 3)), {"ltype": "huffman", "sf": sf})],
            ["lit_huffman_sf%d" % sf, "huf_streams_%d" % (4 if sf else 1)], single=n > 100)
    for n in (6, 7, 8, 9):  # the last of four segments holds 0, 1, 2 and 3 literals
        lits = _text(rng, n, b"xyz")
        add("four_streams_%d" % n, [("comp", lits, [(2, 4, 1)], {"ltype": "huffman", "sf": 1})], ["huf_streams_4"], single=False)
    # RLE literals in 1-, 2- and 3-byte headers
    for sf, n in ((0, 31), (0, 30), (0, 7), (1, 32), (1, 4095), (3, 33), (3, 20000)):
        add("rle_literals_sf%d_%d" % (sf, n), [("comp", b"q" * n, _seqs_for(rng, n - 1, min(50, n // 3)), {"ltype": "rle", "sf": sf})],
            ["lit_rle_sf%d" % sf])
    for sf, n in ((0, 31), (0, 20), (1, 33), (3, 34), (3, 9000)):
        lits = rng.randbytes(n)
        add("raw_literals_sf%d_%d" % (sf, n), [("comp", lits, _seqs_for(rng, n - 1, n // 4) if n else [], {"sf": sf})],
            ["lit_raw_sf%d" % sf])
    # RLE tables: each alone, and all three
    lits = rng.randbytes(400)
    same_ll = [(5, rng.choice((3, 9, 40)), rng.choice((1, 4, 60))) for _ in range(30)]
    same_of = [(rng.choice((1, 4, 9)), rng.choice((3, 9, 40)), 5 + (i & 3)) for i in range(30)]   # offset code 3
    same_ml = [(rng.choice((1, 4, 9)), 7, rng.choice((1, 4, 60))) for _ in range(30)]
    same_all = [(8, 7, 5)] * 30
    same_ll[0], same_of[0], same_ml[0] = (5, 70, 1), (9, 70, 5), (70, 7, 1)   # (offsets stay inside the output)
    for name, seqs, modes in (("ll", same_ll, ("rle", "predefined", "predefined")), ("of", same_of, ("predefined", "rle", "fse")),
                              ("ml", same_ml, ("fse", "predefined", "rle")), ("all", same_all, ("rle", "rle", "rle"))):
        add("rle_table_" + name, [("comp", lits, seqs, {"modes": modes})], ["%s_rle" % t for t in TABLES if name in (t, "all")])
    # FSE-described tables over the accuracy logs
    for al in ((5, 5, 5), (6, 6, 6), (7, 7, 7), (8, 8, 8), (9, 8, 9), (9, 5, 5), (5, 8, 9)):
        lits = _text(rng, 3000, b"etaoin shrdlu")
        seqs = _seqs_for(rng, 2900, 300, offs=(1, 2, 3, 7, 30, 100, 700), mls=(3, 4, 5, 6, 9, 33, 70))
        add("fse_tables_al_%d_%d_%d" % al, [("comp", lits, seqs, {"modes": ("fse",) * 3, "al": al, "ltype": "huffman", "sf": 2})],
            ["ll_fse", "of_fse", "ml_fse"])
    # repeat codes 1, 2, 3 with ll == 0 and ll > 0 (ll == 0 shifts them: 1 -> rep1, 2 -> rep2, 3 -> rep0 - 1)
    lits = rng.randbytes(200)
    reps = [(20, 5, 9), (3, 4, 13), (2, 6, 17)]
    for k in (1, 2, 3):
        reps += [(4, 5, -k), (0, 7, -k), (1, 3, -k), (0, 4, -k)]
    reps += [(0, 5, -3), (0, 5, -3), (2, 4, 30), (0, 9, -3), (0, 3, -1), (0, 3, -2), (5, 3, -3)]
    add("repeat_offsets", [("comp", lits, reps)], ["of_predefined"])
    add("repeat_offsets_fse", [("comp", lits, reps, {"modes": ("fse",) * 3, "al": (5, 5, 5)})], ["of_fse"])
    # match copies: offsets around the 16-byte chunk and the 64-byte round, lengths below and above 64
    lits = rng.randbytes(600)
    seqs = [(70, 3, 1)]
    for off in (1, 2, 15, 16, 17, 63, 64, 65):
        for ml in (3, 15, 17, 63, 64, 65, 130, 200):
            seqs.append((rng.choice((0, 1, 5)), ml, off))
    add("match_copies", [("comp", lits, seqs, {"modes": ("fse", "fse", "fse"), "al": (6, 6, 7)})], ["nseq_1byte"])
    # more than 64 and more than 256 sequences (the execution batches), 2-byte count forced on a small one
    for n, nb in ((65, 1), (100, 2), (127, 1), (128, 2), (257, 2), (700, 2)):
        lits = _text(rng, 3 * n, b"0123456789abcdef")
        add("nseq_%d_%dbyte" % (n, nb), [("comp", lits, _seqs_for(rng, 3 * n - 5, n, rep_every=7), {"ltype": "huffman", "nseq_bytes": nb})],
            ["nseq_%dbyte" % nb])
    # no sequences
    add("nseq_0_raw", [("comp", rng.randbytes(100), [])], ["nseq_0"], single=False)
    add("nseq_0_rle", [("comp", b"r" * 777, [], {"ltype": "rle"})], ["nseq_0", "lit_rle_sf1"])
    add("nseq_0_huffman", [("comp", _text(rng, 2000, b"abcdefg"), [], {"ltype": "huffman", "sf": 2})], ["nseq_0", "lit_huffman_sf2"])
    # frame headers
    small, mid, big = [("comp", rng.randbytes(90), _seqs_for(rng, 80, 9))], \
        [("comp", rng.randbytes(300), _seqs_for(rng, 290, 60))], \
        [("comp", _text(rng, 20000, b"abcdefghij "), _seqs_for(rng, 19000, 1500, mls=(3, 4, 5, 9, 12)), {"ltype": "huffman", "sf": 3})]
    add("hdr_fcs1", small, ["fcs_bytes_1", "single_segment"])
    add("hdr_fcs2", mid, ["fcs_bytes_2"])
    add("hdr_fcs2_max", big, ["fcs_bytes_2"], fcs_bytes=2)
    add("hdr_fcs4", mid, ["fcs_bytes_4"], fcs_bytes=4)
    add("hdr_fcs8", small, ["fcs_bytes_8"], fcs_bytes=8)
    add("hdr_window_no_fcs", mid, ["window_descriptor", "fcs_bytes_0"], single=False)
    add("hdr_window_no_fcs_big", big, ["window_descriptor", "fcs_bytes_0"], single=False)
    for fb in (2, 4, 8):
        add("hdr_window_fcs%d" % fb, mid, ["window_descriptor", "fcs_bytes_%d" % fb], single=False, fcs_bytes=fb)
    for db in (1, 2, 4):
        add("hdr_dict_id_%d" % db, mid, ["dict_id_bytes_%d" % db], did_bytes=db)
        add("hdr_dict_id_%d_window" % db, small, ["dict_id_bytes_%d" % db, "window_descriptor"], did_bytes=db, single=False)
    add("hdr_checksum", mid, ["checksum"], checksum=True)
    add("hdr_checksum_big", big, ["checksum"], checksum=True)
    add("hdr_checksum_window", small, ["checksum", "window_descriptor"], checksum=True, single=False)
    # two blocks: Huffman + FSE tables, then treeless with all three tables repeated
    l1, l2 = _text(rng, 900, b"aabbbcdddde"), _text(rng, 500, b"abcde")
    s1 = _seqs_for(rng, 880, 90, offs=(1, 2, 3, 7, 30, 100), mls=(3, 4, 5, 6, 9, 33))
    s1 = s1[:40] + [(2, 5, -1), (0, 4, -2), (1, 3, -3)] + s1[40:]
    s2, left = [], len(l2)   # drawn from the first block's sequences: every code is in its tables
    while len(s2) < 60:
        q = rng.choice(s1)
        if q[0] > left:
            break
        s2.append(q)
        left -= q[0]
    two = [("comp", l1, s1, {"ltype": "huffman", "sf": 1, "modes": ("fse",) * 3, "al": (6, 5, 6)}),
           ("comp", l2, s2, {"ltype": "treeless", "sf": 1, "modes": ("repeat",) * 3})]
    add("two_blocks_treeless_repeat", two, ["lit_treeless_sf1", "ll_repeat", "of_repeat", "ml_repeat", "frame_multi_block"])
    add("two_blocks_treeless_repeat_checksum", two, ["lit_treeless_sf1", "checksum", "frame_multi_block"], checksum=True)
    add("raw_rle_comp_blocks", [("raw", rng.randbytes(50)), ("rle", 0x41, 300), ("comp", l1, s1, {"ltype": "huffman", "sf": 0}),
                                ("comp", l2[:40], [(3, 5, -1), (0, 5, -2)], {"ltype": "treeless", "sf": 0, "modes": ("repeat", "predefined", "rle")})],
        ["block_raw", "block_rle", "lit_treeless_sf0", "ll_repeat", "frame_multi_block"])
    return out


@functools.lru_cache(maxsize=None)
def rejected_forms():
    """Assembled frames facebook/zstd rejects: Case(name, frame, content length,
    "corrupt" | "unsupported")."""
    rng = random.Random(78)
    out = []

    def add(name, blocks, why="corrupt", **hdr):
        f, want = frame(blocks, **hdr)
        out.append(Case(name, f, len(want), why))

    mid = [("comp", rng.randbytes(300), _seqs_for(rng, 290, 60))]
    add("bad_checksum", mid, checksum=True, bad_checksum=1)
    add("bad_checksum_high_bit", mid, checksum=True, bad_checksum=1 << 31)
    # ll == 0 and code 3 with rep0 == 1: offset 0
    add("rep0_minus_1_is_0", [("comp", rng.randbytes(40), [(5, 4, 1), (0, 4, -3), (3, 3, 2)])], invalid=True)
    add("empty_fourth_stream", [("comp", b"xyzzyx", [(2, 4, 1)], {"ltype": "huffman", "sf": 1, "empty_last_stream": True})],
        single=False)
    # a tree whose longest codes are no pair: weights 2, 2 fill 2^2, but no symbol has weight 1
    add("huffman_no_weight_1", [("comp", bytes(rng.choice((0, 1)) for _ in range(40)), [], {"ltype": "huffman", "sf": 0, "weights": [2, 2]})],
        single=False)
    add("huffman_no_weight_1_4_streams", [("comp", bytes(rng.choice((0, 1, 2)) for _ in range(90)), [(3, 4, 2)],
                                           {"ltype": "huffman", "sf": 1, "weights": [3, 2, 2]})], single=False)
    # a first block that repeats what no block before it set, and is sound otherwise: the hidden block lends
    # the encoder a tree and tables, the frame's length and offsets are those of the block it holds
    l1 = _text(rng, 900, b"aabbbcdddde")
    s1 = _seqs_for(rng, 880, 90, offs=(1, 2, 3, 7, 30), mls=(3, 4, 5, 6, 9, 33))
    prime = ("comp", l1, s1, {"ltype": "huffman", "sf": 1, "modes": ("fse",) * 3, "hidden": True})
    add("first_block_treeless", [prime, ("comp", l1[:400], s1[:20], {"ltype": "treeless", "sf": 1})])
    for t in range(3):
        modes = tuple("repeat" if i == t else "predefined" for i in range(3))
        add("first_block_repeat_" + TABLES[t], [prime, ("comp", l1[:400], s1[:20], {"modes": modes})])
    sound = frame([("comp", l1[:400], s1[:20])])[1]   # the same block with raw literals and predefined tables
    assert all(c.want == len(sound) for c in out[-4:])
    # the same frames behind a sound frame that does set that tree and those tables: a decoder that carried them
    # from frame to frame would decode these, so only its first-block check rejects them
    before, b_want = frame([prime[:3] + ({"ltype": "huffman", "sf": 1, "modes": ("fse",) * 3},)])
    for c in out[-4:]:
        out.append(Case(c.name.replace("first_block", "second_frame"), before + c.frame, len(b_want) + c.want, "corrupt"))
    add("dict_id_nonzero", mid, "unsupported", did_bytes=1, dict_id=7)
    add("dict_id_nonzero_4", mid, "unsupported", did_bytes=4, dict_id=1 << 24)
    return out


@functools.lru_cache(maxsize=None)
def long_count_frames():
    """Blocks of 0x7F00 + 200 and of exactly 0x7F00 sequences: the 3-byte
    sequence count.  Each sequence is one literal and a 3-byte match on the
    repeat offset (1 at the frame's start), so the content is every literal
    four times: 130,848 bytes at the most, within the 128 KiB block limit."""
    rng = random.Random(79)
    out = []
    for n, modes in ((0x7F00 + 200, ("predefined",) * 3), (0x7F00, ("predefined", "rle", "predefined"))):
        f, want = frame([("comp", rng.randbytes(n), [(1, 3, -1)] * n, {"modes": modes})], fcs_bytes=4)
        out.append(Case("nseq_3byte_%d" % n, f, want, ("nseq_3byte",)))
    return out


HUF_SIZES = (40, 200, 700, 1023, 1024, 1500, 5000, 16383, 16384, 20000, 36864)
LEVELS = (-5, 1, 3, 19)


@functools.lru_cache(maxsize=None)
def library_frames():
    """facebook/zstd frames over low-entropy inputs of HUF_SIZES and a dozen
    random sizes at LEVELS: Huffman literals in every size format a block of at
    most 36,864 bytes reaches from the library."""
    rng = random.Random(80)
    sizes = HUF_SIZES + tuple(rng.randrange(40, 36865) for _ in range(12))
    out = []
    for i, n in enumerate(sizes):
        for j, level in enumerate(LEVELS):
            data = low_entropy(rng, i + j, n)
            out.append(Case("lib_%d_L%d_k%d" % (n, level, (i + j) % 4), compress(data, level, checksum=(i + j) % 5 == 0), data, ()))
    return out


@functools.lru_cache(maxsize=None)
def multi_block_frames():
    """140,000-byte letters texts at level 19: several blocks each, and (the
    forms test holds the census to it) treeless literals and repeat tables in
    the later ones."""
    out = []
    for mixed in (False, True):
        data = letters(random.Random(93), 140_000, mixed)
        out.append(Case("lib_140000_L19_k%d" % (3 if mixed else 1), compress(data, 19), data, ("frame_multi_block", "lit_treeless", "of_repeat")))
    return out


@functools.lru_cache(maxsize=None)
def exhaustion_batch():
    """64 letters texts of 36,864 bytes at level 3, as (frame, data): more than
    64 x 4096 sequences in all, past the batch path's sequence area
    (kSeqPerBlock, zstd_fast.hip.h:52, :375)."""
    rng = random.Random(82)
    data = [letters(rng, 36864) for _ in range(64)]
    return [(compress(d, 3), d) for d in data]


@functools.lru_cache(maxsize=None)
def dense_blocks():
    """Eight assembled one-block frames of 9,000 short sequences each (about
    4 decoded bytes a sequence: under 36,864 in all), as (frame, data): more
    than twice kSeqPerBlock a block, which the library never reaches, and
    still the batch path's to take (raw literals, predefined tables)."""
    rng = random.Random(83)
    out = []
    for _ in range(8):
        seqs = [(20, 3, rng.choice((1, 2, 3, 5, 9, 17)))]
        seqs += [(rng.choice((0, 1, 1, 1)), rng.choice((3, 3, 3, 4)), rng.choice((1, 2, 3, 5, 9, 17, -1, -2))) for _ in range(8999)]
        f, want = frame([("comp", rng.randbytes(sum(s[0] for s in seqs) + 5), seqs)])
        assert len(want) <= K_OUT and route(as_is(f, len(want))) == "batch"
        out.append((f, want))
    return out


@functools.lru_cache(maxsize=None)
def exhaustion_batch_mixed():
    """exhaustion_batch() and dense_blocks() three times over (88 zstd blocks),
    with a snappy or a raw block after every fourth: (block, indicator, data)
    for 110 blocks.  The area is sized over all 110, the other codecs' too
    (zstd.hip:136-138), so the dense blocks are what takes the zstd blocks'
    sequences past it; tests/test_zstd_forms.py holds the batch to that."""
    import pyarrow as pa
    zs = exhaustion_batch() + dense_blocks() * 3
    random.Random(84).shuffle(zs)
    out = []
    for i, (f, d) in enumerate(zs):
        out.append((as_is(f, len(d)), 7, d))
        if i % 4 == 3:
            other = d[:300 + 61 * i]
            out.append((pa.Codec("snappy").compress(other, asbytes=True), 1, other) if i % 8 == 3 else (other, 0, other))
    return out


def batch_nseq(blocks):
    """The first-block sequence counts of the zstd blocks among (block, indicator, data)."""
    return [first_block_nseq(bk[len(uvarint(len(d))):])[0] for bk, ind, d in blocks if ind == 7]


@functools.lru_cache(maxsize=None)
def zstd_gpu_corpus():
    """Every valid frame tests/test_zstd_forms_gpu.py decodes on the device."""
    return library_frames() + assembled_forms() + multi_block_frames() + long_count_frames()


def corpus_census(cases) -> collections.Counter:
    c = collections.Counter()
    for case in cases:
        c += census(case.frame)
    return c


# what zstd_gpu_corpus() must hold, each at least twice (tests/test_zstd_forms.py)
COVERAGE_FLOOR = (["lit_huffman_sf%d" % i for i in range(4)] + ["huf_streams_1", "huf_streams_4", "huf_weights_direct", "huf_weights_fse",
                  "lit_treeless", "lit_rle", "lit_raw"] + ["%s_%s" % (t, m) for t in TABLES for m in MODES]
                  + ["nseq_0", "nseq_1byte", "nseq_2byte", "nseq_3byte", "checksum", "window_descriptor", "dict_id_bytes_1", "dict_id_bytes_2",
                     "dict_id_bytes_4", "frame_multi_block"])


def damaged(rng, cases, count=80):
    """`count` damaged frames as (name, frame, decoded length): truncations,
    one-bit flips (inside a Huffman stream, the sequence bitstream, a table
    description or anywhere), wrong decoded lengths -- the census's walk gives
    the offsets."""
    out = []
    cases = [c for c in cases if len(c.want) <= 36864]
    for i in range(count):
        c = cases[i * len(cases) // count]
        f, n = bytearray(c.frame), len(c.want)
        blk = next((b for fr in walk(c.frame) if not fr["skippable"] for b in fr["blocks"] if b["type"] == "compressed"), {})
        kind = ("truncate", "huf_streams", "seq_bits", "tables", "huf_desc", "anywhere", "length")[i % 7]
        if kind == "truncate":
            f = f[:rng.randrange(1, len(f))]
        elif kind == "length":
            n = max(1, n + rng.choice((-1, 1, 7)))
        else:
            a, b = blk.get(kind, (4, len(f)))
            if a >= b:
                a, b = 4, len(f)
            f[rng.randrange(a, b)] ^= 1 << rng.randrange(8)
        out.append(("%s/%s" % (c.name, kind), bytes(f), n))
    return out
