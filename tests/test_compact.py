"""The compaction view without a GPU: the ABI additions
(pbl_compact_struct_layout, the workspace size, the invalid-argument returns,
all before any device call) and pbl_compact_batch_host -- the sequential loop --
against the reference's own recorded cases (tests/golden/compact_iter.json)
and against the Python statement of the rules (compactutil.expected_compact) on
those, on generated inputs and on the status cases."""
import ctypes

import numpy as np
import pytest

from compactutil import (ALL_EVENTS, C, COUNTERS, D, STATUS_EXPECTED, T, assert_compact_is, assert_golden, expected_compact,
                         golden_block, golden_options, host_from_blocks, load_golden, random_block, snapshot_list,
                         status_blocks)
from pebble_amd import _native as N
from pebble_amd.batch import DecodeError
from pebble_amd.compact import compact_host
from pebble_amd.merge import host_struct
from scanutil import result_kvs

G = load_golden()


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_compact_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.CompactInC, N.CompactOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp and n == 15
    assert L.pbl_abi_version() == 9
    # the other lists are what they were
    assert L.pbl_visible_struct_layout(None, 0) == 10 and L.pbl_merge_struct_layout(None, 0) == 11


def test_workspace_bytes_grow_with_the_input_only():
    L = N.lib()
    a, b = L.pbl_compact_workspace_bytes(4, 1000), L.pbl_compact_workspace_bytes(4, 2000)
    assert a % 16 == 0 and b % 16 == 0 and a < b < 2 * a + 4096
    assert L.pbl_compact_workspace_bytes(0, 0) > 0
    assert L.pbl_compact_workspace_bytes(1 << 20, 0) > L.pbl_compact_workspace_bytes(1, 0)


def test_the_fixture_holds_the_counts_it_must():
    cases = G["cases"]
    has = lambda c, k: any(kv[2] == k for kv in c["define"])  # noqa: E731
    assert len(cases) >= 200
    assert sum(1 for c in cases if has(c, "DELSIZED")) >= 12 and sum(1 for c in cases if has(c, "SINGLEDEL")) >= 80
    assert sum(1 for c in cases if c["snapshots"]) >= 80 and sum(1 for c in cases if c["elide"]) >= 20


def _by_options():
    groups = {}
    for n, c in enumerate(G["cases"]):
        groups.setdefault(golden_options(c), []).append((n, c))
    return groups


def test_every_recorded_case_through_the_host_form_and_the_model():
    done = 0
    for (snaps, elide, bottommost), mine in _by_options().items():  # one batch per option set, a block per case
        h = host_from_blocks([golden_block(c, G["kinds"]) for _, c in mine])
        res = compact_host(h, comparer=D, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost)
        assert res["batch"]["status_mask"] == 0, (snaps, elide, bottommost)
        exp = assert_compact_is(res, h, D, snaps, elide, bottommost, (snaps, elide, bottommost))
        for q, (n, c) in enumerate(mine):
            kv0, kv1 = int(res["batch"]["blk_kv_base"][q]), int(res["batch"]["blk_kv_base"][q + 1])
            counts = tuple(int(res[k][q]) for k in COUNTERS)
            assert_golden(c, G["kinds"], result_kvs(res["batch"], q), res["pinned"][kv0:kv1], counts, ("host", n, c["file"]))
            _, e, ecounts = exp[q]
            assert_golden(c, G["kinds"], [x[:4] for x in e], [x[6] for x in e], ecounts, ("model", n, c["file"]))
            done += 1
    assert done == len(G["cases"])


@pytest.mark.parametrize("comparer", [D, T, C], ids=["default", "testkeys", "crdb"])
def test_random_inputs_host_against_model(comparer):
    rng = np.random.default_rng(1234 + comparer)
    events, counted = set(), np.zeros(3, np.int64)
    for n_snaps in (0, 1, 5, 40):
        blocks = [random_block(rng, comparer, 60) for _ in range(3)] + [[]]
        h = host_from_blocks(blocks)
        snaps = snapshot_list(rng, n_snaps)
        for elide in (False, True):
            for bottommost in (False, True):
                res = compact_host(h, comparer=comparer, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost)
                assert res["batch"]["status_mask"] == 0
                assert_compact_is(res, h, comparer, snaps, elide, bottommost, (n_snaps, elide, bottommost), events)
                counted += [int(res[k].sum()) for k in COUNTERS]
                vals = [len(kv[2]) for q in range(3) for kv in result_kvs(res["batch"], q)]
                assert 0 in vals and max(vals) >= 600  # both sides of the 512-byte copy boundary
    assert events == ALL_EVENTS, ALL_EVENTS - events
    assert (counted > 0).all(), counted


def test_statuses_and_their_neighbours():
    h = host_from_blocks(status_blocks())
    for snaps in ((), (8, 25)):
        res = compact_host(h, comparer=D, snapshots=snaps)
        assert res["batch"]["blk_status"].tolist() == STATUS_EXPECTED
        assert_compact_is(res, h, D, snaps, False, False, snaps)
        good = result_kvs(res["batch"], 0)
        assert len(good) >= 3
        for q in range(2, len(STATUS_EXPECTED), 2):  # the good blocks between are unaffected
            assert [len(x[2]) for x in result_kvs(res["batch"], q)] == [len(x[2]) for x in good], q


def test_no_blocks_and_no_kvs():
    for blocks in ([], [[], []]):
        h = host_from_blocks(blocks)
        res = compact_host(h, comparer=D, snapshots=(3,))
        assert res["batch"]["n_kv"] == 0 and res["batch"]["status_mask"] == 0 and len(res["src_kv"]) == 0
        assert_compact_is(res, h, D, (3,), False, False)


def test_invalid_arguments():
    L = N.lib()
    h = host_from_blocks([[(b"a", 5 << 8 | 1, b"v")]])
    with pytest.raises(DecodeError, match="INVALID_ARG"):
        compact_host(h, comparer=D, snapshots=(9, 3), sort_snapshots=False)
    assert compact_host(h, comparer=D, snapshots=(9, 3))["batch"]["n_kv"] == 1  # the wrapper sorts
    keep = []
    cin = N.CompactInC(host_struct(h, keep), 1, D, 0, None, 0)
    tot = N.TotalsC()
    bases = [np.zeros(2, np.uint64) for _ in range(3)]
    status = np.zeros(1, np.uint32)
    o = N.DecodeOutC()
    o.blk_kv_base, o.blk_key_base, o.blk_val_base = (b.ctypes.data for b in bases)
    o.blk_status, o.totals = status.ctypes.data, ctypes.addressof(tot)
    co = N.CompactOutC(o, None, None, None, None, None, None)
    assert L.pbl_compact_batch_host(ctypes.byref(cin), ctypes.byref(co), 0) == N.PBL_OK and tot.n_kv == 1
    for flags in (N.PBL_COMPACT_SIZED, 0x8, 0x80000000):
        assert L.pbl_compact_batch_host(ctypes.byref(cin), ctypes.byref(co), flags) == N.PBL_INVALID_ARG
    assert L.pbl_compact_batch_host(None, ctypes.byref(co), 0) == N.PBL_INVALID_ARG
    assert L.pbl_compact_batch_host(ctypes.byref(cin), None, 0) == N.PBL_INVALID_ARG
    bad = N.CompactInC(host_struct(h, keep), 1, 3, 0, None, 0)
    assert L.pbl_compact_batch_host(ctypes.byref(bad), ctypes.byref(co), 0) == N.PBL_INVALID_ARG
    nolist = N.CompactInC(host_struct(h, keep), 1, D, 0, None, 2)
    assert L.pbl_compact_batch_host(ctypes.byref(nolist), ctypes.byref(co), 0) == N.PBL_INVALID_ARG
    # the device entry points refuse the same before any device call (no workspace is needed to say so)
    ws = ctypes.c_void_p(16)
    assert L.pbl_compact_size(ctypes.byref(cin), ctypes.byref(co), ws, 1 << 40, N.PBL_COMPACT_SIZED, None) == N.PBL_INVALID_ARG
    assert L.pbl_compact_batch(ctypes.byref(cin), ctypes.byref(co), ws, 1 << 40, 0x10, None) == N.PBL_INVALID_ARG
    assert L.pbl_compact_size(ctypes.byref(cin), ctypes.byref(co), None, 1 << 40, 0, None) == N.PBL_INVALID_ARG
    assert L.pbl_compact_size(ctypes.byref(cin), ctypes.byref(co), ctypes.c_void_p(8), 1 << 40, 0, None) == N.PBL_INVALID_ARG
    assert L.pbl_compact_size(ctypes.byref(cin), ctypes.byref(co), ws, 16, 0, None) == N.PBL_INVALID_ARG


def test_overflow_writes_sizes_and_nothing_else():
    L = N.lib()
    h = host_from_blocks([[(b"a", 5 << 8 | 1, b"value"), (b"b", 4 << 8 | 1, b"w")]])
    keep = []
    cin = N.CompactInC(host_struct(h, keep), 1, D, 0, None, 0)
    tot = N.TotalsC()
    arrays = {k: np.full(8, 0xEE, dt) for k, dt in (("blk_kv_base", np.uint64), ("blk_key_base", np.uint64),
                                                     ("blk_val_base", np.uint64), ("blk_status", np.uint32),
                                                     ("trailer", np.uint64), ("key_off", np.uint32), ("val_off", np.uint32),
                                                     ("key_bytes", np.uint8), ("val_bytes", np.uint8))}
    o = N.DecodeOutC()
    for k, a in arrays.items():
        setattr(o, k, a.ctypes.data)
    o.totals = ctypes.addressof(tot)
    o.kv_cap, o.key_cap, o.val_cap = 1, 8, 8  # one KV too few
    co = N.CompactOutC(o, None, None, None, None, None, None)
    assert L.pbl_compact_batch_host(ctypes.byref(cin), ctypes.byref(co), 0) == N.PBL_OK
    assert tot.status_mask == 1 << N.PBL_OVERFLOW and (tot.n_kv, tot.key_bytes, tot.val_bytes) == (2, 2, 6)
    assert arrays["blk_kv_base"][:2].tolist() == [0, 2]
    assert (arrays["trailer"] == 0xEE).all() and (arrays["key_bytes"] == 0xEE).all()
