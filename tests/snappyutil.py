"""Snappy blocks for the snappy decoders' tests (golang/snappy's block format:
a uvarint decoded length, then literal and copy elements), in pure Python:

  * lit() / c1() / c2() / c4(): an assembler that writes elements from explicit
    parts, for what an encoder never emits (3- and 4-byte literal lengths,
    non-canonical literal headers, 4-byte offsets, 2-byte-offset copies of
    length 1 to 3); assemble() runs an element list and returns
    (block, decoded);
  * parse() / census(): a walk of a block's bytes that decodes them and counts
    the element forms present, so a test can state which forms its corpus
    holds on which route instead of assuming them;
  * route(): which of the device's three routes a block of n compressed bytes
    decoding to D takes (pebble_amd/csrc/snappy_dec.hip.h's sn4_walkable and
    snappy2_kernel's conditions, restated);
  * route wrappers that move a case to another route without touching its
    elements -- a run of copies behind it, or a literal and a run of copies
    in front of it, which puts the case's own elements at output offsets that
    need the high half of sn_qent's 16-bit fields;
  * corpus(), rejected() and damaged(): what tests/test_snappy_forms.py holds
    to the oracle and to a census floor on the CPU, and
    tests/test_snappy_forms_gpu.py decodes on the device.

The ground truth for every block is oracle.snappy_decode (snappy.Decode
restated in C); parse() is a second, independent decoder."""
import collections
import functools
import random

import numpy as np

# snappy_dec.hip.h / physical.hip
K_S4_IN = 36864        # kS4In: the walk's input limit
K_S4_SPAN = 32768      # kS4Span: the walk's output limit
K_SN_WALK_MIN = 64     # kSnWalkMin: smaller outputs are not walked
K_SN_IN = 32768        # kSnIn: the LDS route's staged input
LDS_D_MAX = 0xFFFF     # the LDS route's 16-bit output offsets
K_SN_Q = 592           # kSnQ: elements per round, LDS route
K_S4_Q = 768           # kS4Q: elements per round, walked route
ROUTE_NAMES = ("walk", "lds", "global")


def uvarint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append(n & 0x7F | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def bitmap_floor(n: int) -> int:
    """The walk leaves a 16-byte header and a bit per input byte in the output region."""
    return 16 + 4 * ((n + 31) // 32)


def route(n: int, D: int) -> str:
    if 8 <= n <= K_S4_IN and K_SN_WALK_MIN <= D <= K_S4_SPAN and D >= bitmap_floor(n):   # sn4_walkable
        return "walk"
    if n <= K_SN_IN and D <= LDS_D_MAX:                                                   # snappy2_kernel
        return "lds"
    return "global"


# ---- the assembler ---------------------------------------------------------------
def min_form(length: int) -> int:
    x = length - 1
    return 0 if x < 60 else next(k for k in (1, 2, 3, 4) if x < 1 << (8 * k))


def lit_header(length: int, form=None) -> bytes:
    """A literal's tag and length bytes: form 0 holds length - 1 in the tag,
    forms 1..4 in that many bytes behind the tag 59 + form."""
    x = length - 1
    if form is None:
        form = min_form(length)
    if form == 0:
        assert 0 <= x < 60
        return bytes([x << 2])
    assert 0 <= x < 1 << (8 * form)
    return bytes([(59 + form) << 2]) + x.to_bytes(form, "little")


def lit(data: bytes, form=None) -> bytes:
    return lit_header(len(data), form) + bytes(data)


def c1(off: int, length: int) -> bytes:
    assert 4 <= length <= 11 and 0 <= off < 2048
    return bytes([1 | (length - 4) << 2 | (off >> 8) << 5, off & 0xFF])


def c2(off: int, length: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= off < 1 << 16
    return bytes([2 | (length - 1) << 2]) + off.to_bytes(2, "little")


def c4(off: int, length: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= off < 1 << 32
    return bytes([3 | (length - 1) << 2]) + off.to_bytes(4, "little")


COPY = {1: c1, 2: c2, 4: c4}


# ---- the parser --------------------------------------------------------------------
class Corrupt(Exception):
    pass


# s, d: the element's input and output offsets; kind 0 literal, 1 / 2 / 4 copy;
# form: a literal's length bytes; depth: a copy's chain depth (see walk)
Elem = collections.namedtuple("Elem", "s d kind form length off depth")


def walk(src: bytes, s: int, D):
    """Decode the elements of src from offset s on (D: the decoded length the
    block claims, or None to take what comes): (elements, output), or Corrupt
    for each of snappy.Decode's ErrCorrupt reasons.

    A copy's chain depth is 1 + the deepest copy among its source bytes,
    literal bytes counting 0.  An overlapping copy (offset < length) has depth
    1 whatever it reads: the decoders never follow a chain through one, they
    run it in place."""
    n = len(src)
    limit = D if D is not None else 1 << 22
    out = bytearray()
    dep = np.zeros(limit + 1, np.uint16)
    elems = []
    while s < n:
        t, d, s0 = src[s], len(out), s
        kind = (0, 1, 2, 4)[t & 3]
        if kind == 0:
            x, form = t >> 2, 0
            s += 1
            if x >= 60:
                form = x - 59
                if s + form > n:
                    raise Corrupt("literal header cut")
                x = int.from_bytes(src[s: s + form], "little")
                s += form
            ln = x + 1                       # (Go's int: 2^32 does not wrap)
            if ln > n - s or ln > limit - d:
                raise Corrupt("literal length")
            out += src[s: s + ln]
            s += ln
            elems.append(Elem(s0, d, 0, form, ln, 0, 0))
            continue
        h = {1: 2, 2: 3, 4: 5}[kind]
        if s + h > n:
            raise Corrupt("copy header cut")
        if kind == 1:
            ln, off = 4 + ((t >> 2) & 7), (t & 0xE0) << 3 | src[s + 1]
        else:
            ln, off = 1 + (t >> 2), int.from_bytes(src[s + 1: s + h], "little")
        s += h
        if off == 0 or off > d or ln > limit - d:
            raise Corrupt("copy offset or length")
        if off >= ln:
            out += out[d - off: d - off + ln]
            depth = 1 + int(dep[d - off: d - off + ln].max())
        else:
            out += (bytes(out[d - off: d]) * (ln // off + 1))[:ln]
            depth = 1
        dep[d: d + ln] = depth
        elems.append(Elem(s0, d, kind, 0, ln, off, depth))
    if D is not None and len(out) != D:
        raise Corrupt("output short of the decoded length")
    return elems, bytes(out)


def header(block: bytes):
    """(D, header bytes) of a block, or Corrupt (snappy.DecodedLen)."""
    x = 0
    for i, b in enumerate(block[:10]):
        x |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            if x > 0xFFFFFFFF:
                raise Corrupt("decoded length over 32 bits")
            return x, i + 1
    raise Corrupt("unterminated decoded length")


def parse(block: bytes):
    """(D, elements, decoded bytes) of a whole block, or Corrupt."""
    D, used = header(block)
    if D > 1 << 22:
        raise Corrupt("decoded length past this parser's limit")
    elems, out = walk(block, used, D)
    return D, elems, out


def decode(block: bytes):
    """The decoded bytes, or None: oracle.snappy_decode's contract."""
    try:
        return parse(block)[2]
    except Corrupt:
        return None


def assemble(elements):
    """Run a list of encoded elements: (block, decoded)."""
    body = b"".join(elements)
    _, out = walk(body, 0, None)
    return uvarint(len(out)) + body, out


@functools.lru_cache(maxsize=None)
def census(block: bytes) -> collections.Counter:
    """The element forms of one (valid) block, counted from its bytes (cached:
    callers add it to their own counters and leave it unchanged)."""
    D, elems, _ = parse(block)
    c = collections.Counter()
    for e in elems:
        if e.kind == 0:
            c["lit_form_%d" % e.form] += 1
            if e.form != min_form(e.length):
                c["lit_noncanonical"] += 1
            c["lit_len_lt16" if e.length < 16 else "lit_len_16_256" if e.length <= 256 else "lit_len_gt256"] += 1
        else:
            c["copy_%d" % e.kind] += 1
            if e.length <= 3:
                c["copy_len_1_3"] += 1
            c["off_lt16" if e.off < 16 else "off_16" if e.off == 16 else "off_eq_d" if e.off == e.d else "off_17_up"] += 1
            if e.off >= 32768:
                c["off_ge_32768"] += 1       # (bit 15 of a 2-byte offset)
            if e.off >= 65536:
                c["off_ge_65536"] += 1       # (only a 4-byte offset holds it)
            c["chain_1" if e.depth == 1 else "chain_2_8" if e.depth <= 8 else "chain_9_64" if e.depth <= 64
              else "chain_gt64"] += 1
        if e.d >= 32768:
            c["elem_at_32768"] += 1
        if e.d >= 65536:
            c["elem_at_65536"] += 1
    for q in (K_SN_Q, K_S4_Q):
        k = len(elems)
        c["nel_%s_%d" % ("lt" if k < q else "eq" if k == q else "gt2" if k > 2 * q else "gt", q)] += 1
        if k > q:
            c["nel_over_%d" % q] += 1
    c["blocks"] += 1
    return c


LIT_FORMS = ["lit_form_%d" % f for f in range(5)]
COPY_KINDS = ["copy_1", "copy_2", "copy_4"]
OFF_CLASSES = ["off_lt16", "off_16", "off_17_up", "off_eq_d"]
# what every route must hold (tests/test_snappy_forms.py); the walked route
# ends at output offset 32768 and so holds no element at or past it
FLOOR = {r: LIT_FORMS + COPY_KINDS + OFF_CLASSES + ["lit_noncanonical", "lit_len_lt16", "lit_len_16_256", "lit_len_gt256",
                                                  "copy_len_1_3", "chain_1", "chain_2_8", "chain_gt64"]
         for r in ROUTE_NAMES}
FLOOR["walk"] += ["nel_over_%d" % K_S4_Q, "nel_eq_%d" % K_S4_Q, "nel_gt2_%d" % K_S4_Q]
FLOOR["lds"] += ["elem_at_32768", "off_ge_32768", "nel_over_%d" % K_SN_Q, "nel_eq_%d" % K_SN_Q, "nel_gt2_%d" % K_SN_Q]
FLOOR["global"] += ["elem_at_32768", "elem_at_65536", "off_ge_32768", "off_ge_65536", "nel_over_%d" % K_SN_Q, "nel_over_%d" % K_S4_Q]


# ---- cases and route wrappers --------------------------------------------------------
# body: the elements' bytes (no length header); want: what they decode to
Case = collections.namedtuple("Case", "name body want")
# one block on one route: `wrapper` names how the case got there
Wrapped = collections.namedtuple("Wrapped", "name wrapper route block want")


def case(name, elements) -> Case:
    body = b"".join(elements)
    return Case(name, body, walk(body, 0, None)[1])


PAD = c2(1, 64)   # 64 more of the last output byte
FRONT = bytes(range(0xB0, 0xC0))


@functools.lru_cache(maxsize=None)
def _big_literal() -> bytes:
    return lit(random.Random(77).randbytes(32769))


def as_is(c: Case):
    return uvarint(len(c.want)) + c.body, c.want


def _behind(c: Case, past: int):
    """Runs of c2(1, 64) behind the case until D crosses `past`."""
    if not c.want:
        return None
    k = -(-(past + 1 - len(c.want)) // 64)
    if k <= 0:
        return None                 # (already past it: as_is is that block)
    want = c.want + c.want[-1:] * (64 * k)
    return uvarint(len(want)) + c.body + PAD * k, want


def _front(c: Case, at: int):
    """A literal and runs of c2(1, 64) first: the case's own elements start at
    output offset >= `at`."""
    k = -(-(at - len(FRONT)) // 64)
    want = FRONT + FRONT[-1:] * (64 * k) + c.want
    return uvarint(len(want)) + lit(FRONT) + PAD * k + c.body, want


def behind_lds(c):
    return _behind(c, 32768)


def behind_global(c):
    return _behind(c, 65535)


def front_lds(c):
    return _front(c, 32768)


def front_global(c):
    return _front(c, 65536)


def front_literal(c):
    """A 32,769-byte literal first: the global route by n, not by D."""
    big = _big_literal()
    return uvarint(32769 + len(c.want)) + big + c.body, big[-32769:] + c.want


# wrapper -> the route it is for (as_is: whichever the block takes)
WRAPPERS = ((as_is, None), (behind_lds, "lds"), (front_lds, "lds"), (behind_global, "global"), (front_global, "global"),
            (front_literal, "global"))


def wrapped(c: Case):
    """The case on every route it can reach: a wrapper whose block would not
    take the route it is for (more input than kSnIn on the LDS route, say) is
    left out, so each case carries the list of routes it takes."""
    out = []
    for wrap, want_route in WRAPPERS:
        r = wrap(c)
        if r is None:
            continue
        block, want = r
        got = route(len(block), len(want))
        if want_route is None or got == want_route:
            out.append(Wrapped(c.name, wrap.__name__, got, block, want))
    return out


# ---- the corpus ------------------------------------------------------------------------
LIT_LENGTHS = (1, 59, 60, 61, 255, 256, 257, 300, 5000)
OFFSETS = (1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 1023, 1024, 2047, 16384)
COPY_LENGTHS = {1: (4, 11), 2: (1, 64), 4: (1, 64)}
CHAIN_DEPTHS = (2, 8, 100, 1500)
ELEMENT_COUNTS = (591, 592, 593, 767, 768, 769, 1535, 1536, 1537)


def chain(rng, depth, shift):
    """Copies of copies, `depth` deep.  shift 0: every hop copies the whole
    of the one before (offset == length == 16).  shift 3: a hop copies the one
    before from its fourth byte on, three bytes shorter each time; when a hop
    would fall under 4 bytes the next is 64 wide again and reads across the
    short hops behind it (a source that straddles elements)."""
    width = 16 if shift == 0 else 32 if depth > 500 else 64
    els, ln = [lit(rng.randbytes(max(width, 64)))], width
    els.append(c2(ln, ln))
    for _ in range(depth - 1):
        if shift and ln - shift < 4:
            ln = width
            els.append(c2(ln, ln))
        else:
            els.append(c2(ln - shift, ln - shift))
            ln -= shift
    return els


def counted(rng, count, kind):
    """`count` elements: "lits" 1- to 3-byte literals; "mixed" short literals
    and copies of all three kinds; "big" a 5000-byte literal and long copies,
    decoding past 32768 bytes."""
    if kind == "lits":
        return [lit(rng.randbytes(1 + i % 3)) for i in range(count)]
    if kind == "mixed":
        els = [lit(rng.randbytes(24))]
        for i in range(1, count):
            els.append((lit(rng.randbytes(1 + i % 5)), c1(5 + i % 19, 4 + i % 8), c2(1 + i % 23, 1 + i % 9),
                        c4(3 + i % 20, 2 + i % 7))[i % 4])
        return els
    ln = min(64, 55000 // count)
    els = [lit(rng.randbytes(5000))]
    for i in range(1, count):
        els.append(lit(rng.randbytes(2)) if i % 8 == 0 else (c2, c4)[i % 2](70 + 37 * (i % 97), ln - i % 3))
    return els


def _to_length(rng, D, first=1000, off=500):
    """A literal and c2(off, 64) copies decoding to exactly D bytes."""
    rest = D - first
    return [lit(rng.randbytes(first))] + [c2(off, 64)] * (rest // 64) + ([c2(off, rest % 64)] if rest % 64 else [])


def _at_floor(below: int):
    """1-byte literals, a of them with 4 length bytes and b inline, whose
    decoded length is the walk's bitmap floor less `below` (64 at the least)."""
    for a in range(40, 120):
        for b in range(0, 60):
            D, n = a + b, 1 + 6 * a + 2 * b
            if D >= K_SN_WALK_MIN and D == bitmap_floor(n) - below:
                return [lit(bytes([65 + i % 26]), 4) for i in range(a)] + [lit(bytes([97 + i % 26])) for i in range(b)]
    raise AssertionError("no such block")


def _input_length(rng, n_total, D=32768):
    """n_total compressed bytes decoding to D: 1-byte literals with 4 length
    bytes (5 bytes of overhead each), inline ones (1 each) and one long literal."""
    over = n_total - D - len(uvarint(D)) - 3        # (the long literal's header: 3 bytes)
    a, b = over // 5, over % 5
    return ([lit(bytes([65 + i % 26]), 4) for i in range(a)] + [lit(bytes([97 + i % 26])) for i in range(b)]
            + [lit(rng.randbytes(D - a - b), 2)])


def encoder_blocks(rng):
    import pyarrow as pa
    vocab = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 9))) + b" " for _ in range(300)]
    text = b"".join(rng.choice(vocab) for _ in range(9000))
    out = []
    for name, data in (("text_30000", text[:30000]), ("text_50000", text[:50000]), ("ab_9000", b"ab" * 4500),
                       ("random_2000", rng.randbytes(2000))):
        raw = pa.Codec("snappy").compress(data, asbytes=True)
        out.append(Case("encoder/" + name, raw[len(uvarint(len(data))):], data))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Every valid case, as a tuple of Case."""
    rng = random.Random(20240)
    out = []
    # every literal form x length
    for form in range(5):
        for ln in LIT_LENGTHS:
            if ln - 1 < (60 if form == 0 else 1 << (8 * form)):
                out.append(case("lit/form%d_len%d" % (form, ln), [lit(rng.randbytes(ln), form)]))
    # every copy kind x offset x both ends of its length range
    for kind, mk in COPY.items():
        lo, hi = COPY_LENGTHS[kind]
        for off in OFFSETS:
            if kind == 1 and off >= 2048:
                continue
            out.append(case("copy%d/off%d" % (kind, off), [lit(rng.randbytes(off + 5)), mk(off, lo), mk(off, hi)]))
        out.append(case("copy%d/off_d" % kind, [lit(rng.randbytes(33)), mk(33, lo), mk(33 + lo, hi)]))
    # literals only a 3- or 4-byte length holds (the global route by n and by D)
    for form in (3, 4):
        out.append(case("lit/form%d_len70000" % form, [lit(rng.randbytes(70000), form)]))
    # offsets near the top of each route's output: past 16384 on the walked route, with
    # bit 15 set on the LDS route, past 16 bits on the global route
    run = [lit(rng.randbytes(200))] + [c2(200, 64)] * 500                                  # d = 32200
    out.append(case("far/walk", run + [c2(32000, 64), c4(32199, 64), c1(2047, 11), c4(32339, 1), c2(32340, 64)]))
    run = [lit(rng.randbytes(200))] + [c2(200, 64)] * 640                                  # d = 41160
    out.append(case("far/lds", run + [c2(40000, 64), c4(40001, 33), c2(41257, 5), c4(32768, 64), c2(32767, 64), c4(41390, 3),
                                      c2(41393, 64)]))
    run = [lit(rng.randbytes(200))] + [c2(200, 64)] * 1030                                 # d = 66120
    out.append(case("far/global", run + [c2(65535, 64), c4(65535, 64), c4(65536, 64), c4(66000, 7), c4(66319, 64), c4(65537, 1),
                                         c4(66384, 2)]))
    # copies of copies
    for depth in CHAIN_DEPTHS:
        for shift in (0, 3):
            out.append(case("chain/depth%d_shift%d" % (depth, shift), chain(rng, depth, shift)))
    # 1-byte copies: n several times D
    out.append(case("onebyte/c4_off1", [lit(b"q")] + [c4(1, 1)] * 200))
    out.append(case("onebyte/c2_off1", [lit(b"r")] + [c2(1, 1)] * 300))
    out.append(case("onebyte/c4_c2_off5", [lit(b"stuvw")] + [c4(5, 1), c2(5, 1)] * 250))
    # element counts around kSnQ and kS4Q
    for count in ELEMENT_COUNTS:
        for kind in ("lits", "mixed", "big"):
            out.append(case("count/%s_%d" % (kind, count), counted(rng, count, kind)))
    # the route boundaries
    out.append(Case("edge/empty", b"", b""))
    out.append(case("edge/n7", [lit(b"ab"), PAD]))
    out.append(case("edge/n8", [lit(b"abc"), PAD]))
    out.append(case("edge/D63", [lit(rng.randbytes(63), 1)]))
    out.append(case("edge/D64", [lit(rng.randbytes(64), 1)]))
    out.append(case("edge/D_at_floor", _at_floor(0)))
    out.append(case("edge/D_below_floor", _at_floor(1)))
    for D in (32768, 32769, 65535, 65536):
        out.append(case("edge/D%d" % D, _to_length(rng, D)))
    out.append(case("edge/n32768", [lit(rng.randbytes(32702), 2)] + [c2(100, 64)] * 20))
    out.append(case("edge/n32769", [lit(rng.randbytes(32703), 2)] + [c2(100, 64)] * 20))
    out.append(case("edge/n36864", _input_length(rng, 36864)))
    out.append(case("edge/n36865", _input_length(rng, 36865)))
    out += encoder_blocks(rng)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wrapped_corpus():
    """Every corpus case on every wrapper that takes it where it should."""
    return tuple(w for c in corpus() for w in wrapped(c))


def route_census(blocks):
    """{route: Counter} over Wrapped blocks, counted by the parser."""
    cen = {r: collections.Counter() for r in ROUTE_NAMES}
    for w in blocks:
        cen[w.route] += census(w.block)
    return cen


def sample_by_cell(blocks, per_cell=1):
    """A small sample that still holds every (route, census cell) the blocks
    hold: for each cell the cheapest blocks (fewest decoded bytes) that have
    it, in the blocks' own order for ties."""
    cells = collections.defaultdict(list)
    for i, w in enumerate(blocks):
        for k in census(w.block):
            cells[(w.route, k)].append((len(w.want), i))
    keep = set()
    for held in cells.values():
        keep.update(i for _, i in sorted(held)[:per_cell])
    return [blocks[i] for i in sorted(keep)]


# ---- blocks snappy.Decode rejects -----------------------------------------------------
WRAPPED_LENGTH = b"\xfc\xff\xff\xff\xff"    # a literal of 2^32 bytes: 32-bit arithmetic wraps it to 0
Rejected = collections.namedtuple("Rejected", "name route block")


def _reject_prefix(r):
    """Valid elements that put what follows on route r, and their output length."""
    if r == "walk":
        pre = lit(bytes(range(100)))
    elif r == "lds":
        pre = lit(FRONT) + PAD * 512          # d = 32784
    else:
        pre = lit(FRONT * 4) + PAD * 1023     # d = 65536: below 0x10004
    return pre, len(walk(pre, 0, None)[1])


@functools.lru_cache(maxsize=None)
def rejected():
    """One block per ErrCorrupt reason on each route (route None: the length
    header itself is bad, no route is chosen)."""
    out = []
    for r in ROUTE_NAMES:
        pre, d = _reject_prefix(r)

        def add(name, tail, more, front=b""):
            out.append(Rejected("%s/%s" % (name, r), r, uvarint(d + more) + front + pre + tail))

        heads = {"lit1": lit_header(200, 1), "lit2": lit_header(200, 2), "lit3": lit_header(200, 3), "lit4": lit_header(200, 4),
                 "c1": c1(5, 4), "c2": c2(5, 4), "c4": c4(5, 4)}
        for hn, h in heads.items():
            for cut in range(1, len(h)):
                add("cut_%s_%d" % (hn, cut), h[:cut], 10)
        for kind, mk in COPY.items():
            add("offset_0_c%d" % kind, mk(0, 4), 4)
        add("offset_d_plus_1_c4", c4(d + 1, 4), 4)
        if d + 1 < 1 << 16:
            add("offset_d_plus_1_c2", c2(d + 1, 4), 4)
        add("offset_bit31", c4(0x80000004, 4), 4)
        add("offset_0x10004", c4(0x10004, 4), 4)
        add("copy_past_D", PAD, 10)
        add("literal_past_D", lit(bytes(20)), 10)
        add("output_short_of_D", lit(bytes(5)), 10)
        add("literal_past_input", lit_header(50) + bytes(10), 50)
        add("wrapped_length_first", b"", 0, front=WRAPPED_LENGTH)
        add("wrapped_length_middle", WRAPPED_LENGTH + lit(bytes(10)), 10)
        add("wrapped_length_last", WRAPPED_LENGTH, 0)
    # a copy before any output, then enough to choose the route
    rng = random.Random(5)
    for r, ln in (("walk", 100), ("lds", 10), ("global", 70000)):
        out.append(Rejected("copy_before_output/" + r, r, uvarint(4 + ln) + c2(1, 4) + lit(rng.randbytes(ln))))
    # the wrapped length next to a 70,000-byte literal (the global route by n and by D)
    big = lit(rng.randbytes(70000))
    out.append(Rejected("wrapped_length_behind_70000/global", "global", uvarint(70000) + big + WRAPPED_LENGTH))
    out.append(Rejected("wrapped_length_before_70000/global", "global", uvarint(70000) + WRAPPED_LENGTH + big))
    out.append(Rejected("length_unterminated", None, b"\xff" * 11 + lit(b"abc")))
    out.append(Rejected("length_cut", None, b"\x80"))
    out.append(Rejected("length_over_32_bits", None, b"\x80\x80\x80\x80\x10" + lit(b"abc")))
    return tuple(out)


def damaged(rng, cases, count=80):
    """`count` damaged blocks as (name, block): one-bit flips past the length
    varint, and truncations (the varint stays whole, so every block still has
    a decoded length and a route)."""
    out = []
    cases = [c for c in cases if c.body]
    for i in range(count):
        c = cases[i * len(cases) // count]
        block, _ = as_is(c)
        used = len(uvarint(len(c.want)))
        kind = ("flip", "flip", "truncate")[i % 3]
        b = bytearray(block)
        if kind == "truncate":
            b = b[:rng.randrange(used, len(b))]
        else:
            b[rng.randrange(used, len(b))] ^= 1 << rng.randrange(8)
        out.append(("%s/%s" % (c.name, kind), bytes(b)))
    return out


def rewrap_front(block: bytes, at: int):
    """A (possibly damaged) block's elements behind the front pad: its decoded
    length grows by the pad's."""
    D, used = header(block)
    k = -(-(at - len(FRONT)) // 64)
    return uvarint(D + len(FRONT) + 64 * k) + lit(FRONT) + PAD * k + block[used:]
