"""Table bloom filters without a GPU: the host forms (pbl_filter_probe_host,
pbl_bloom_build_host, pbl_seek_prefix_batch_host) -- the same filter_core.hip.h
the kernels instantiate -- against the reference's recorded data
(tests/golden/filter.json: TestHash, TestSmallBloomFilter, the filter block of
the reference's bloom table) and against the plain-Python restatement of the
format (tests/filterutil.py); the ABI additions and every invalid-argument
return."""
import ctypes

import numpy as np
import pytest

import filterutil as FU
import oracle
from pebble_amd import _native as N
from pebble_amd import filter as F
from pebble_amd.seek import pack_keys, seek_host
from tableutil import table_bytes

G = FU.load_golden()
CASES = FU.filter_cases()


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_filter_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.FilterSetC, N.FilterQueriesC, N.FilterOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp
    assert N.STATUS_NAMES[N.PBL_CORRUPT_FILTER] == "CORRUPT_FILTER" and N.PBL_CORRUPT_FILTER == 15
    assert L.pbl_abi_version() == 9


def test_hash_vectors_of_the_reference():
    keys = [bytes.fromhex(v["key"]) for v in G["hash"]]
    assert len(keys) == 41
    _, hs, _ = F.probe_host([b""], keys, N.PBL_CMP_DEFAULT)
    assert hs.tolist() == [v["hash"] for v in G["hash"]]
    assert [FU.bloom_hash(k) for k in keys] == hs.tolist()


def test_hash_of_every_tail_length_with_sign_extended_bytes():
    keys = FU.edge_keys()
    assert {len(k) for k in keys} == set(range(41))
    _, hs, _ = F.probe_host([b""], keys, N.PBL_CMP_DEFAULT)
    assert hs.tolist() == [FU.bloom_hash(k) for k in keys]
    # sign extension matters: the unsigned reading of a tail byte >= 0x80 differs
    u = (((0xBC9F1D34 ^ 0xC6A4A793) + 0x80) * 0xC6A4A793) & FU.M32
    assert FU.bloom_hash(b"\x80") != u ^ (u >> 24)


def test_small_filter_bytes_and_answers():
    s = G["small"]
    keys = [k.encode() for k in s["keys"]]
    f = F.build_host(keys, N.PBL_CMP_DEFAULT, s["bits_per_key"])
    assert f.hex() == s["filter_hex"] and len(f) == 69
    assert FU.build(keys, FU.D, s["bits_per_key"]) == f
    names = sorted(s["answers"])
    may, _, st = F.probe_host([f], [k.encode() for k in names], N.PBL_CMP_DEFAULT)
    assert [bool(m) for m in may[0]] == [s["answers"][k] for k in names]
    assert st.tolist() == [N.PBL_OK]


@pytest.mark.parametrize("name,flt,members", CASES, ids=[c[0] for c in CASES])
def test_probe_equals_the_restatement(name, flt, members):
    keys = FU.probe_keys(members)
    may, hs, st = F.probe_host([flt], keys, N.PBL_CMP_DEFAULT)
    e_may, e_hs, e_st = FU.expected_probe([flt], keys, FU.D)
    assert may.reshape(-1).tolist() == e_may and hs.tolist() == e_hs and st.tolist() == e_st
    n_lines, _, status = FU.parse(flt)
    if name.startswith("bpk"):  # no false negative, and the builder is the restatement's
        assert all(m == N.PBL_FILTER_MAY for m in may[0][:min(60, len(members))])
        bpk = int(name[3:name.index("_")])
        assert F.build_host(members, N.PBL_CMP_DEFAULT, bpk) == flt
    if name == "probes0":
        assert set(may[0].tolist()) == {N.PBL_FILTER_MAY}
    if name in ("probes30", "probes255"):
        assert 0 in may[0].tolist() and N.PBL_FILTER_MAY in may[0].tolist()
    if name in ("len0", "len5"):
        assert not may.any() and status == FU.OK
    if status != FU.OK:
        assert set(may[0].tolist()) == {N.PBL_FILTER_MAY | N.PBL_FILTER_BAD} and st[0] == N.PBL_CORRUPT_FILTER


def test_named_mode_and_ids_past_the_filters():
    flts = [CASES[0][1], CASES[4][1], b"", CASES[-1][1]]
    keys = FU.probe_keys(CASES[4][2], 20)
    which = [(i * 5) % 6 for i in range(len(keys))]  # 4 and 5 are past n_filters
    may, hs, st = F.probe_host(flts, keys, N.PBL_CMP_DEFAULT, which=which)
    e_may, e_hs, e_st = FU.expected_probe(flts, keys, FU.D, which)
    assert may.tolist() == e_may and hs.tolist() == e_hs and st.tolist() == e_st
    assert all(m == (N.PBL_FILTER_MAY | N.PBL_FILTER_BAD) for m, w in zip(may, which) if w >= 4)
    assert st.tolist() == [0, 0, 0, N.PBL_CORRUPT_FILTER]


def test_all_pairs_is_filter_major():
    flts = [c[1] for c in CASES[:5]]
    keys = FU.probe_keys(CASES[1][2], 7)
    may, _, _ = F.probe_host(flts, keys, N.PBL_CMP_DEFAULT)
    assert may.shape == (5, len(keys))
    for f, flt in enumerate(flts):
        one, _, _ = F.probe_host([flt], keys, N.PBL_CMP_DEFAULT)
        assert may[f].tolist() == one[0].tolist()
    assert may.reshape(-1).tolist() == FU.expected_probe(flts, keys, FU.D)[0]


def test_builder_drops_a_hash_equal_to_the_one_before_it():
    keys = [b"a", b"a", b"b", b"b", b"b", b"a"]
    f = F.build_host(keys, N.PBL_CMP_DEFAULT, 512)
    assert f == FU.build(keys, FU.D, 512) == FU.build([b"a", b"b", b"a"], FU.D, 512)
    assert FU.parse(f)[0] == 3  # three hashes at 512 bits each; six would give seven lines
    assert FU.parse(F.build_host([b"a", b"b", b"a", b"b", b"a", b"b"], N.PBL_CMP_DEFAULT, 512))[0] == 7
    assert F.build_host([], N.PBL_CMP_DEFAULT, 10) == b""


@pytest.mark.parametrize("comparer", [N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB])
def test_the_probed_bytes_are_the_split_prefix(comparer):
    if comparer == N.PBL_CMP_TESTKEYS:
        a5, a9, other = b"a@5", b"a@9", b"b@5"
    else:
        ver = lambda w: w.to_bytes(8, "big") + b"\x09"  # noqa: E731
        a5, a9, other = b"a\x00" + ver(5), b"a\x00" + ver(9), b"b\x00" + ver(5)
    f = F.build_host([a5], comparer, 10)
    assert f == FU.build([a5], comparer, 10) == F.build_host([a5[:FU.split(comparer, a5)]], N.PBL_CMP_DEFAULT, 10)
    may, hs, _ = F.probe_host([f], [a5, a9, other], comparer)
    assert hs[0] == hs[1] == FU.prefix_hash(comparer, a9) and hs[2] != hs[0]
    assert may[0].tolist() == [1, 1, 0]
    # versions of one prefix are one hash: the duplicate rule keeps one
    assert F.build_host([a5, a9], comparer, 10) == f


def _bloom_table_host(name):
    """The table's data blocks through the oracle's host walk (footer, row index,
    row decode), as the decoded-batch layout."""
    data = table_bytes(name + ".sst")
    f = oracle.parse_footer(data[-61:], len(data))
    ck = f["checksum_type"]
    st, top = oracle.index_block_row(oracle.table_block(data, f["index"], ck))
    assert st == 0
    blocks = [oracle.table_block(data, (o, ln), ck) for o, ln, _p in top]
    off, pos = [], 0
    for b in blocks:
        off.append(pos)
        pos += (len(b) + 15) // 16 * 16
    buf = np.zeros(pos + 16, np.uint8)
    for o, b in zip(off, blocks):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    h = oracle.rowblk_decode_batch(buf, np.array(off, np.uint64), np.array([len(b) for b in blocks], np.uint32), 0)
    assert not h["blk_status"].any()
    return data, f, h


def _user_keys(h):
    from seekutil import block_keys
    return [k for b in range(len(h["blk_status"])) for k in block_keys(h, b)]


@pytest.fixture(scope="module")
def bloom_table():
    data, f, h = _bloom_table_host("h_bloom_no_compression")
    t = G["tables"]["h_bloom_no_compression"]
    flt = oracle.table_block(data, tuple(t["filter_handle"]), f["checksum_type"])
    return h, _user_keys(h), flt, t


def test_reference_table_filter_rebuilt_byte_for_byte(bloom_table):
    h, keys, flt, t = bloom_table
    assert len(keys) == 1710 and len(flt) == 2245
    assert FU.parse(flt) == (t["n_lines"], t["n_probes"], FU.OK) == (35, 6, 0)
    assert F.build_host(keys, N.PBL_CMP_DEFAULT, 10) == flt
    snappy = table_bytes("h_bloom_snappy.sst")
    o, ln = G["tables"]["h_bloom_snappy"]["filter_handle"]
    assert snappy[o:o + ln] == flt  # filter blocks are stored uncompressed


def test_reference_table_no_false_negative_and_the_recorded_false_positives(bloom_table):
    h, keys, flt, t = bloom_table
    may, _, _ = F.probe_host([flt], keys, N.PBL_CMP_DEFAULT)
    assert may.all()
    m = [b"m!" + i.to_bytes(4, "little") for i in range(10000)]
    may, _, _ = F.probe_host([flt], m, N.PBL_CMP_DEFAULT)
    assert int(may.sum()) == t["false_positives_m"] == 88


def test_seek_prefix_host_is_the_seek_behind_the_filter(bloom_table):
    h, keys, flt, _ = bloom_table
    q = keys[::37] + [k + b"!" for k in keys[::41]] + [b"", b"\xff\xff"] + \
        [b"m!" + i.to_bytes(4, "little") for i in range(300)]
    kv, blk, fl = seek_host(h, q, comparer=N.PBL_CMP_DEFAULT, filter=flt)
    kv0, blk0, fl0 = seek_host(h, q, comparer=N.PBL_CMP_DEFAULT)
    may, _, _ = F.probe_host([flt], q, N.PBL_CMP_DEFAULT)
    out = may[0] == 0
    assert out.any() and not out.all()
    assert (fl[out] == N.PBL_SEEK_FILTERED).all() and (kv[out] == N.PBL_SEEK_NONE).all() and (blk[out] == 0).all()
    assert (kv[~out] == kv0[~out]).all() and (blk[~out] == blk0[~out]).all() and (fl[~out] == fl0[~out]).all()
    # an exact hit is never filtered: a bloom filter has no false negatives
    assert not (out & ((fl0 & N.PBL_SEEK_EXACT) != 0)).any()
    # a corrupt filter excludes nothing and marks every answer
    bad = FU.with_trailer(flt, n_lines=36)
    kv, blk, fl = seek_host(h, q, comparer=N.PBL_CMP_DEFAULT, filter=bad)
    assert (kv == kv0).all() and (blk == blk0).all() and (fl == (fl0 | N.PBL_SEEK_BAD_BLOCK)).all()
    # a filter that holds nothing excludes everything
    kv, blk, fl = seek_host(h, q, comparer=N.PBL_CMP_DEFAULT, filter=b"")
    assert (kv == N.PBL_SEEK_NONE).all() and (fl == N.PBL_SEEK_FILTERED).all()


class _Args:
    """A syntactically valid argument set over host memory: every device call
    below must return before it touches any of it."""

    def __init__(self):
        self.arr = np.zeros(64, np.uint64)
        p = self.arr.ctypes.data
        self.set = N.FilterSetC(p, p, 1)
        self.q = N.FilterQueriesC(p, p, None, 4, N.PBL_CMP_DEFAULT)
        self.out = N.FilterOutC(p, p, p)

    def call(self, fn="pbl_filter_probe", s=True, q=True, o=True):
        a = [ctypes.byref(self.set) if s else None, ctypes.byref(self.q) if q else None,
             ctypes.byref(self.out) if o else None]
        return getattr(N.lib(), fn)(*a, None) if fn == "pbl_filter_probe" else getattr(N.lib(), fn)(*a)


@pytest.mark.parametrize("fn", ["pbl_filter_probe", "pbl_filter_probe_host"])
def test_invalid_arguments_return_before_any_device_call(fn):
    for miss in ("s", "q", "o"):
        assert _Args().call(fn, **{miss: False}) == N.PBL_INVALID_ARG
    a = _Args()
    a.out.may = None
    assert a.call(fn) == N.PBL_INVALID_ARG
    a = _Args()
    a.q.key_off = None
    assert a.call(fn) == N.PBL_INVALID_ARG
    a = _Args()
    a.q.comparer = 3
    assert a.call(fn) == N.PBL_INVALID_ARG
    a = _Args()
    a.q.n = 0
    assert a.call(fn) == N.PBL_OK  # no launch
    a = _Args()
    a.set.n_filters = 0
    assert a.call(fn) == N.PBL_OK


def test_builder_and_prefix_seek_argument_errors():
    L = N.lib()
    kb, ko = pack_keys([b"a", b"b"])
    out = np.zeros(256, np.uint8)
    ln = ctypes.c_uint64(0)
    build = lambda *a: L.pbl_bloom_build_host(*a)  # noqa: E731
    assert build(kb.ctypes.data, ko.ctypes.data, 2, 3, 10, out.ctypes.data, 256, ctypes.byref(ln)) == N.PBL_INVALID_ARG
    assert build(kb.ctypes.data, ko.ctypes.data, 2, 0, 0, out.ctypes.data, 256, ctypes.byref(ln)) == N.PBL_INVALID_ARG
    assert build(kb.ctypes.data, None, 2, 0, 10, out.ctypes.data, 256, ctypes.byref(ln)) == N.PBL_INVALID_ARG
    assert build(kb.ctypes.data, ko.ctypes.data, 2, 0, 10, out.ctypes.data, 256, None) == N.PBL_INVALID_ARG
    assert build(kb.ctypes.data, ko.ctypes.data, 2, 0, 10, out.ctypes.data, 68, ctypes.byref(ln)) == N.PBL_OVERFLOW
    assert ln.value == 69 == L.pbl_bloom_build_bound(2, 10)
    assert L.pbl_bloom_build_bound(0, 10) == 0
    assert build(kb.ctypes.data, ko.ctypes.data, 2, 0, 10, out.ctypes.data, 69, ctypes.byref(ln)) == N.PBL_OK

    arr = np.zeros(64, np.uint64)
    p = arr.ctypes.data
    d = N.DecodeOutC()
    for f in ("kv_flags", "key_off", "key_bytes", "blk_kv_base", "blk_key_base", "blk_status"):
        setattr(d, f, p)
    so = N.SeekOutC(p, p, p)
    ws = np.zeros(4096 + 16, np.uint8)
    wp = (ws.ctypes.data + 15) // 16 * 16

    def dev(q, flt=p, w=wp, wn=4096):
        return L.pbl_seek_prefix_batch(ctypes.byref(d), 4, ctypes.byref(q), flt, 69, ctypes.byref(so),
                                       ctypes.c_void_p(w) if w else None, wn, None)

    def host(q, flt=p):
        return L.pbl_seek_prefix_batch_host(ctypes.byref(d), 4, ctypes.byref(q), flt, 69, ctypes.byref(so))

    ok = lambda: N.SeekQueriesC(p, p, None, 4, N.PBL_CMP_DEFAULT, N.PBL_SEEK_GE, 0)  # noqa: E731
    for call in (dev, host):
        assert call(ok(), flt=None) == N.PBL_INVALID_ARG  # no filter
        q = ok()
        q.op = N.PBL_SEEK_LT
        assert call(q) == N.PBL_INVALID_ARG
        q = ok()
        q.block = p  # per-block mode
        assert call(q) == N.PBL_INVALID_ARG
        q = ok()
        q.comparer = 3
        assert call(q) == N.PBL_INVALID_ARG
        q = ok()
        q.n = 0
        assert call(q) == N.PBL_OK
    assert dev(ok(), w=None, wn=0) == N.PBL_INVALID_ARG  # table mode needs the fence
    assert dev(ok(), wn=16) == N.PBL_INVALID_ARG
