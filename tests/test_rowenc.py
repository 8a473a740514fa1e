"""The row-block encoder's host form (pbl_rowenc_batch_host) without a GPU:
the reference's own table reproduced byte for byte, the recorded block lengths
of sstable/testdata/writer_v3, the host form against the Python model of
tests/rowencutil.py, the round trip through the oracle's decoder, and the ABI
(struct layouts, workspace size, invalid arguments)."""
import ctypes

import numpy as np
import pytest

from pebble_amd import _native as N
from pebble_amd.rowenc import RowEncOptions, encode_host
from rowencutil import (HAMLET_OPTS, SET, assert_round_trip, assert_same, block_bytes, edge_cases, hamlet, host_of,
                        load_golden, model_encode, random_cases, tr)


@pytest.fixture(scope="module")
def hamlet_table():
    return hamlet()


def test_reference_table_byte_for_byte(hamlet_table):
    """sstable/testdata/h-no-compression-sst: its 1710 KVs as one stream, with
    the options it was written with, give its 14 data blocks exactly."""
    blocks, host = hamlet_table
    assert len(blocks) == 14 and host["n_kv"] == 1710
    r = encode_host(host, HAMLET_OPTS)
    assert r["n_blocks"] == 14 and r["status_mask"] == 0
    for b, want in enumerate(blocks):
        assert block_bytes(r, b) == want, b
    assert r["block_off"].tolist() == [int(x) for x in np.cumsum([0] + [(len(b) + 15) // 16 * 16 for b in blocks])[:-1]]
    assert int(r["block_n_kv"].sum()) == 1710 and r["block_first_kv"][0] == 0
    assert_same(r, model_encode(host, HAMLET_OPTS), "hamlet")


@pytest.mark.parametrize("target,n_blocks", [(4096, 7), (1024, 27)])
def test_reference_table_is_sensitive_to_the_flush_rule(hamlet_table, target, n_blocks):
    blocks, host = hamlet_table
    r = encode_host(host, RowEncOptions(16, target, 90))
    assert r["n_blocks"] == n_blocks
    assert block_bytes(r, 0) != blocks[0]


def test_recorded_block_lengths():
    """writer_v3's `layout` at block-size=1: 22, 22, 22 with the value prefix
    byte (the default format), 21, 21, 21 for LevelDB."""
    cases = load_golden()["cases"]
    assert sorted(c["table_format"] or "" for c in cases) == ["", "LevelDB"]
    for c in cases:
        v3 = c["table_format"] is None
        assert c["data_block_lengths"] == ([22, 22, 22] if v3 else [21, 21, 21])
        kvs = [(k["key"].encode(), tr(k["seq"], k["kind"]), k["value"].encode()) for k in c["kvs"]]
        r = encode_host(host_of([kvs]), RowEncOptions(16, 1, 90, value_prefix=v3, obsolete=v3))
        assert r["block_len"].tolist() == c["data_block_lengths"], c["cmd"]
        assert r["block_n_kv"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("case", random_cases() + edge_cases(), ids=lambda c: c[0])
def test_host_form_against_the_model_and_round_trip(case):
    name, opts, streams = case
    host = host_of(streams)
    r = encode_host(host, opts)
    assert_same(r, model_encode(host, opts), name)
    assert_round_trip(host, r, opts, ctx=name)


def test_rule_2_trap_shares_trailer_bytes():
    """"k"#1,SET before "k\\x01.." shares 2 bytes without the value prefix
    format, 1 with it (the cap is Split(prev) = 1)."""
    kvs = [(b"k", tr(1, SET), b"a"), (b"k\x01zz", tr(7), b"b")]
    for vp, shared in ((False, 2), (True, 1)):
        r = encode_host(host_of([kvs]), RowEncOptions(16, 4096, 90, value_prefix=vp))
        blk = block_bytes(r, 0)
        second = 3 + 9 + (2 if vp else 1)  # the first entry: 3 varints, "k" + trailer, the stored value
        assert blk[second] == shared, (vp, blk[second])


def test_lowest_level_tombstones_need_a_predecessor():
    """Rule 4, stated without either loop: makeAddPointDecisionV3 returns before C3
    for a table's first point key, so a tombstone that opens a stream is not
    written obsolete at the lowest level; every later one is."""
    from rowencutil import DEL, DELSIZED, SINGLEDEL
    tomb = [(b"a", tr(9, DEL), b""), (b"b", tr(9, SINGLEDEL), b""), (b"c", tr(9, DELSIZED), b"\x05"), (b"d", tr(9), b"v"),
            (b"d", tr(8, DEL), b"")]
    lowest = RowEncOptions(2, 4096, 90, value_prefix=True, obsolete=True, lowest_level=True)
    r = encode_host(host_of([tomb, tomb[1:]]), lowest)
    assert r["obsolete"].tolist() == [0, 1, 1, 0, 1] + [0, 1, 0, 1]
    r = encode_host(host_of([tomb]), RowEncOptions(2, 4096, 90, value_prefix=True, obsolete=True))
    assert r["obsolete"].tolist() == [0, 0, 0, 0, 1]  # only the DEL under the SET of its own user key
    forced = [(k, t, v, N.PBL_KV_OBSOLETE) for k, t, v in tomb[:1]] + tomb[1:]
    assert encode_host(host_of([forced]), lowest)["obsolete"].tolist() == [1, 1, 1, 0, 1]  # forceObsolete reaches the first


def test_overflow_reports_every_size():
    host = host_of([[(b"%04d" % i, tr(3), b"v" * 20) for i in range(40)], [(b"a", tr(1), b"")]])
    opts = RowEncOptions(4, 128, 90)
    full = encode_host(host, opts)
    assert full["n_blocks"] > 3 and not full["status_mask"]
    for caps in ({"block_cap": 2}, {"blocks_cap": 64}, {"block_cap": 0, "blocks_cap": 0}):
        r = encode_host(host, opts, **caps)
        assert r["status_mask"] == 1 << N.PBL_OVERFLOW, caps
        for k in ("n_blocks", "block_bytes", "n_restarts"):
            assert r[k] == full[k], (caps, k)
        assert np.array_equal(r["stream_block_base"], full["stream_block_base"])


def test_struct_layouts_match_library():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_rowenc_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.RowEncOptsC, N.RowEncInC, N.RowEncTotalsC, N.RowEncOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp


def test_workspace_and_invalid_arguments():
    L = N.lib()
    assert L.pbl_rowenc_workspace_bytes(0, 0) % 16 == 0
    assert L.pbl_rowenc_workspace_bytes(10, 1000) > L.pbl_rowenc_workspace_bytes(10, 10) >= 256
    host = host_of([[(b"a", tr(1), b"v")]])
    from pebble_amd.batch import DecodeError
    for bad in (RowEncOptions(0, 100, 90), RowEncOptions(16, 0, 90), RowEncOptions(16, 1 << 31, 90),
                RowEncOptions(16, 100, 90, comparer=3), RowEncOptions(16, 100, 90, obsolete=True),
                RowEncOptions(16, 100, 90, value_prefix=False, obsolete=True, lowest_level=True)):
        with pytest.raises(DecodeError, match="INVALID_ARG"):
            encode_host(host, bad)
    # device entry points refuse before any device call
    o = RowEncOptions().c_struct()
    assert L.pbl_rowenc_size(None, ctypes.byref(o), None, None, 0, None) == N.PBL_INVALID_ARG
    assert L.pbl_rowenc_batch(None, ctypes.byref(o), None, None, 0, 0, None) == N.PBL_INVALID_ARG
