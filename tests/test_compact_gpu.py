"""The compaction view on the device (pbl_compact_size / pbl_compact_batch,
pebble_amd/csrc/compact.hip) over batches decoded on the device.  The expected
result is the host's over to_host() of the same batch (pbl_compact_batch_host,
the sequential loop; every array, per-KV output, counter and status compared
exactly), the Python statement of the rules (compactutil.expected_compact) and
the reference's own recorded cases (tests/golden/compact_iter.json)."""
import ctypes

import numpy as np
import pytest

from compactutil import (COUNTERS, D, DEL, DELSIZED, MERGE, SET, SETWITHDEL, SINGLEDEL, STATUS_EXPECTED, assert_compact_is,
                         assert_golden, assert_same, device_result, golden_block, golden_options, group, load_golden,
                         status_blocks, tr, uvarint)
from pebble_amd import _native as N
from pebble_amd.compact import compact, compact_host, compact_tables
from pebble_amd.rowblk import Writer
from scanutil import result_kvs

pytestmark = pytest.mark.gpu


def dev_decode(blocks):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0))


def row_block(kvs, restart=16):
    w = Writer(restart)
    for kv in kvs:
        w.add(kv[0], kv[1], kv[2])
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def dev_batch(blocks, restart=16):
    """The blocks as row blocks, decoded on the device; a KV's fourth element is
    OR-ed into its kv_flags."""
    import torch
    d = dev_decode([corrupt(row_block([(b"x", 1 << 8 | 1, b"")])) if b is None else row_block(b, restart) for b in blocks])
    extra = [kv[3] if len(kv) > 3 else 0 for b in blocks for kv in (b or [])]
    if any(extra):
        d.kv_flags[: len(extra)] |= torch.tensor(extra, dtype=torch.uint8, device="cuda")
    return d


def check(d, comparer, snaps=(), elide=False, bottommost=False, ctx="", python=True, h=None):
    """Device against pbl_compact_batch_host (everything) and against the Python
    model.  Returns (device result, the input's host arrays)."""
    h = d.to_host() if h is None else h
    r = device_result(compact(d, comparer=comparer, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost))
    assert_same(r, compact_host(h, comparer=comparer, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost), ctx)
    if python:
        assert_compact_is(r, h, comparer, snaps, elide, bottommost, ctx)
    return r, h


# ---- 1. the reference's recorded cases: all of them as one batch, a block per case ---------------
def test_every_recorded_case_as_one_batch():
    g = load_golden()
    cases = g["cases"]
    assert len(cases) >= 200
    d = dev_batch([golden_block(c, g["kinds"]) for c in cases], restart=4)
    h = d.to_host()
    done = 0
    for opt in sorted({golden_options(c) for c in cases}):
        snaps, elide, bottommost = opt
        r, _ = check(d, D, snaps, elide, bottommost, opt, python=False, h=h)
        assert r["batch"]["status_mask"] == 0
        for q, c in enumerate(cases):
            if golden_options(c) != opt:
                continue
            kv0, kv1 = int(r["batch"]["blk_kv_base"][q]), int(r["batch"]["blk_kv_base"][q + 1])
            assert_golden(c, g["kinds"], result_kvs(r["batch"], q), r["pinned"][kv0:kv1], tuple(int(r[k][q]) for k in COUNTERS),
                          (q, c["file"], opt))
            done += 1
    assert done == len(cases)


# ---- 2. every state live across a tile boundary ---------------------------------------------------
BLOCK_KVS = 512  # every boundary block holds exactly two tiles, so that block b's position 256 is flat index 512 b + 256


def boundary_blocks():
    """Per case a block of exactly 512 KVs: 250 one-version keys, then one key
    whose versions occupy the block's positions 250.. so that the named state is
    the incoming state of position 256, then more one-version keys.  A block
    starts at a multiple of 512 of the batch's flat KV index, over which the
    kernels tile, so position 256 is the first KV of a tile in every block.
    Sequence numbers fall from 100 (position 250) so that snapshots (94, 92)
    cut stripes at positions 256 / 257 and 258 / 259 as well.
    Returns {name: (state without elision, state with elision)} and the blocks."""
    sized = lambda n: uvarint(len(b"key") + n)  # noqa: E731
    pend, pend_e = "singledel pending", "singledel pending under elision"
    heads = {
        "seeking": ([SINGLEDEL, SET, SINGLEDEL, MERGE, SINGLEDEL, SET, MERGE, MERGE, SET, DEL], None, "seeking", "seeking"),
        "set looking": ([SET, MERGE, SET, SETWITHDEL, MERGE, SET, SET, MERGE, SINGLEDEL, SET], None, "set looking",
                        "set looking"),
        "merging": ([MERGE] * 9 + [SETWITHDEL, SET], None, "merging", "merging"),
        "merging to the end": ([MERGE] * 11, None, "merging", "merging"),
        "singledel pending": ([SINGLEDEL] * 8 + [DELSIZED, SET], None, pend, pend_e),
        "singledel pending to the end": ([SINGLEDEL] * 9, None, pend, pend_e),
        "singledel consumes": ([SINGLEDEL] * 7 + [SET, SET, MERGE], None, pend, pend_e),
        "delsized holding": ([DELSIZED] * 7 + [SET, SET], [sized(3)] * 6 + [sized(2), b"ab", b"cd"], "delsized holding",
                             "skipping"),
        "delsized holding, missized": ([DELSIZED] * 7 + [MERGE, SET], [sized(3)] * 7 + [b"ab", b"cd"], "delsized holding",
                                       "skipping"),
        "delsized holding to the end": ([DELSIZED] * 8, [sized(n) for n in range(8)], "delsized holding", "skipping"),
        "delsized empty": ([DELSIZED] * 7 + [DELSIZED, SET, SET], [sized(1)] + [b""] * 6 + [sized(1), b"a", b"b"],
                           "delsized empty", "skipping"),
        "delsized empty to a del": ([DELSIZED] * 7 + [SINGLEDEL, SET], [b""] * 9, "delsized empty", "skipping"),
        "skipping": ([DEL, SET, MERGE, SINGLEDEL, SET, DELSIZED, SET, MERGE, SET], None, "skipping", "skipping"),
    }
    blocks = []
    for name, (kinds, vals, _, _) in heads.items():
        pad = [(b"a%04d" % i, tr(5 + i % 3, (SET, DEL, MERGE)[i % 3]), b"p%d" % i) for i in range(250)]
        blk = pad + group(b"key", kinds, 100, vals) + group(b"m", [MERGE, SET], 9) + group(b"z", [SINGLEDEL], 3)
        blk += [(b"zz%04d" % i, tr(5 + i % 3, (SET, DEL, MERGE)[i % 3]), b"q%d" % i) for i in range(BLOCK_KVS - len(blk))]
        assert len(blk) == BLOCK_KVS and len(kinds) > 7
        blocks.append(blk)
    return {n: h[2:] for n, h in heads.items()}, blocks


def test_states_across_a_tile_boundary():
    from compactutil import STATES, state_before
    states, blocks = boundary_blocks()
    d = dev_batch(blocks)
    h = d.to_host()
    # the named state is live at a tile boundary of the flat KV index, strictly inside the key's versions
    seen = set()
    for q, (name, (plain, elided)) in enumerate(states.items()):
        kv0, kvs = int(h["blk_kv_base"][q]), result_kvs(h, q)
        at = 256 - kv0 % 256
        assert kv0 == q * BLOCK_KVS and (kv0 + at) % 256 == 0, name
        assert kvs[at - 1][0] == kvs[at][0] == kvs[at + 1][0] == b"key", name
        assert (state_before(kvs, at), state_before(kvs, at, elide=True)) == (plain, elided), name
        seen |= {plain, elided}
    assert seen == set(STATES)
    n_results = set()
    for snaps in ((), (94,), (92, 94), (3, 6, 8, 95, 97)):
        for elide in (False, True):
            for bottommost in (False, True):
                r, _ = check(d, D, snaps, elide, bottommost, (snaps, elide, bottommost), h=h)
                assert r["batch"]["status_mask"] == 0
                n_results.add(r["batch"]["n_kv"])
    assert len(n_results) > 4


# ---- 3. one group longer than a tile and than a chunk of 256 tiles --------------------------------
def long_blocks(n=70000):
    one = lambda s: bytes([s % 251])  # noqa: E731
    merge = [(b"the key", tr(n - i, MERGE if i < n - 1 else SET), one(n - i)) for i in range(n)]
    sd = [(b"the key", tr(n - i, SINGLEDEL if i < n - 1 else DEL), b"") for i in range(n)]
    return [merge, sd]


@pytest.fixture(scope="module")
def long_batch():
    d = dev_batch(long_blocks())
    return d, d.to_host()


def test_one_group_of_70000_versions(long_batch):
    d, h = long_batch
    r, _ = check(d, D, (), False, False, "70000", h=h)
    kvs = result_kvs(r["batch"], 0)
    assert len(kvs) == 1 and kvs[0][1] == tr(70000, SET) and len(kvs[0][2]) == 70000
    assert kvs[0][2][:3] == bytes([1, 2, 3]) and r["n_src"].tolist() == [70000, 1]
    # 69,999 SINGLEDELs passed over, the first one's key kept, the DEL after them decides
    kvs = result_kvs(r["batch"], 1)
    assert len(kvs) == 1 and kvs[0][1] == tr(70000, DEL) and r["src_kv"].tolist() == [0, 70000]
    assert r["n_ineffectual"].tolist() == [0, 70000 - 1]
    check(d, D, (), True, True, "70000, elided", python=False, h=h)


def test_one_group_of_70000_versions_in_300_stripes(long_batch):
    d, h = long_batch
    snaps = [200 + 233 * i for i in range(300)]
    r, _ = check(d, D, snaps, False, False, "70000, 300 snapshots", h=h)
    assert r["batch"]["blk_kv_base"].tolist() == [0, 301, 602] and r["pinned"].tolist() == ([0] + [1] * 300) * 2
    check(d, D, snaps, True, True, "70000, 300 snapshots, elided", python=False, h=h)


# ---- 4. many small blocks, statuses between good ones ----------------------------------------------
def test_a_thousand_one_kv_blocks():
    kinds = (SET, DEL, MERGE, SINGLEDEL, SETWITHDEL, DELSIZED)
    d = dev_batch([[(b"k%04d" % i, tr(1 + i % 7, kinds[i % 6]), b"" if kinds[i % 6] in (DEL, SINGLEDEL) else uvarint(i))]
                   for i in range(1000)], restart=1)
    h = d.to_host()
    for elide, bottommost in ((False, False), (True, True)):
        r, _ = check(d, D, (4,), elide, bottommost, ("1000 blocks", elide), h=h)
        assert 0 < r["batch"]["n_kv"] <= 1000


def test_statuses_between_good_blocks():
    d = dev_batch(status_blocks())
    for snaps in ((), (8, 25)):
        r, _ = check(d, D, snaps, False, False, snaps)
        exp = list(STATUS_EXPECTED)
        exp[1] = N.PBL_CORRUPT_NO_RESTARTS  # (the block that arrives with a status of its own)
        assert r["batch"]["blk_status"].tolist() == exp


# ---- 5. the unsized call, and overflow ---------------------------------------------------------------
def _direct(d, cap, flags, snaps=()):
    """pbl_compact_batch without a size call before it, into a result of capacity cap."""
    import torch
    from pebble_amd.batch import DecodedBatch
    L = N.lib()
    nb, n_kv = d.n_blocks, int(d.to_host()["n_kv"])
    out = DecodedBatch.allocate(nb, cap, "cuda", entry_off=d.entry_off is not None, restarts=False)
    for t in (out.trailer, out.key_bytes, out.val_bytes, out.key_off, out.val_off):
        t.fill_(0x5A)
    ws = torch.empty(int(L.pbl_compact_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device="cuda")
    sd = torch.tensor(list(snaps), dtype=torch.int64, device="cuda") if snaps else None
    per_kv = [torch.zeros(max(cap.kv, 1), dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.uint8)]
    counts = torch.zeros((3, nb), dtype=torch.int32, device="cuda")
    cin = N.CompactInC(d.c_struct(), nb, D, n_kv, sd.data_ptr() if sd is not None else None, len(snaps))
    co = N.CompactOutC(out.c_struct(), *[t.data_ptr() for t in per_kv], *[counts[i].data_ptr() for i in range(3)])
    rc = L.pbl_compact_batch(ctypes.byref(cin), ctypes.byref(co), ctypes.c_void_p(ws.data_ptr()), ws.numel(), flags,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.PBL_OK
    torch.cuda.synchronize()
    t = out.read_totals()
    return out, per_kv, counts, t


def test_the_unsized_call_equals_the_sized_one():
    from pebble_amd.batch import Capacity
    _, blocks = boundary_blocks()
    d = dev_batch(blocks)
    ref = compact(d, comparer=D, snapshots=(92, 94), elide_tombstones=True)
    want = device_result(ref)
    b = want["batch"]
    cap = Capacity(kv=b["n_kv"], key=b["key_bytes_total"], val=b["val_bytes_total"], rst=0)
    out, per_kv, counts, t = _direct(d, cap, N.PBL_COMPACT_ELIDE_TOMBSTONES, (92, 94))
    assert int(t.status_mask) == 0 and int(t.n_kv) == cap.kv
    got = {"batch": out.to_host(), "src_kv": per_kv[0].cpu().numpy().view(np.uint64)[: cap.kv],
           "n_src": per_kv[1].cpu().numpy().view(np.uint32)[: cap.kv], "pinned": per_kv[2].cpu().numpy()[: cap.kv],
           **{k: counts[i].cpu().numpy().view(np.uint32) for i, k in enumerate(COUNTERS)}}
    assert_same(got, want, "unsized")


def test_overflow_writes_sizes_and_nothing_else():
    from pebble_amd.batch import Capacity
    _, blocks = boundary_blocks()
    d = dev_batch(blocks[:3])
    b = device_result(compact(d, comparer=D))["batch"]
    for cap in (Capacity(kv=b["n_kv"] - 1, key=b["key_bytes_total"], val=b["val_bytes_total"], rst=0),
                Capacity(kv=b["n_kv"], key=b["key_bytes_total"], val=b["val_bytes_total"] - 1, rst=0)):
        out, per_kv, _, t = _direct(d, cap, 0)
        assert int(t.status_mask) == 1 << N.PBL_OVERFLOW
        assert (int(t.n_kv), int(t.key_bytes), int(t.val_bytes)) == (b["n_kv"], b["key_bytes_total"], b["val_bytes_total"])
        assert out.blk_kv_base.cpu().numpy().view(np.uint64).tolist() == b["blk_kv_base"].tolist()
        assert (out.trailer.cpu().numpy() == 0x5A).all() and (out.key_bytes.cpu().numpy() == 0x5A).all()
        assert (out.val_bytes.cpu().numpy() == 0x5A).all() and not per_kv[0].any()


# ---- 6. compact_tables: decode -> scan -> merge -> compact -----------------------------------------
class BlocksTable:
    """What merge_scan needs of a table, over row blocks decoded on the device."""

    def __init__(self, kvs, per_block, restart):
        self.d = dev_decode([row_block(kvs[i:i + per_block], restart) for i in range(0, len(kvs), per_block)])

    def comparer(self):
        return D

    def scan(self, lowers, uppers, hide_obsolete_points=False):
        from pebble_amd.scan import scan
        return scan(self.d, lowers, uppers, comparer=D, hide_obsolete_points=hide_obsolete_points)


def test_compact_tables_over_three_row_tables_and_a_columnar_one():
    from keyspanutil import with_range_dels
    from pebble_amd.merge import merge_host
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    kinds = [SET, MERGE, DEL, MERGE, SINGLEDEL, SET, MERGE, DELSIZED, SETWITHDEL, SINGLEDEL, SET]
    kvs = []
    for i in range(900):
        k = kinds[(i * 7 + i // 5) % len(kinds)]
        key = b"ggg%03d" % (i // 6)
        val = b"" if k in (DEL, SINGLEDEL) else uvarint(len(key) + 4 + i % 2) if k == DELSIZED else b"v%03d" % (i % 1000)
        kvs.append((key, tr(3000 - i, k), val))
    data = table_bytes("find_val_sep_000011.sst")
    col = Table(data)
    assert col.comparer() == D
    tables = [BlocksTable(kvs[r::3], (130, 256, 77)[r], (1, 4, 16)[r]) for r in range(3)] + [col]
    lo, up = [None, b"ggg050", b"ggg100"], [None, b"ggg100", b"ggg100\x00"]
    hosts = [t.scan(lo, up).batch.to_host() for t in tables]
    union = merge_host(hosts, comparer=D)[0]
    assert union["n_kv"] > 900
    for snaps, elide, bottommost in (((), False, False), ((2500, 2800, 2900), True, True)):
        got = device_result(compact_tables(tables, lo, up, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost))
        assert_same(got, compact_host(union, comparer=D, snapshots=snaps, elide_tombstones=elide, bottommost=bottommost), snaps)
        exp = assert_compact_is(got, union, D, snaps, elide, bottommost, snaps)
        assert len(exp[0][1]) > 100 and 0 < len(exp[1][1]) < len(exp[0][1]) and got["batch"]["status_mask"] == 0
    # range deletions and range keys are not silently dropped
    spans = [(b"a", b"z", [(100 << 8 | 15, b"", b"")])]
    with pytest.raises(ValueError, match="range deletions"):
        compact_tables([Table(with_range_dels(data, spans))], [None], [None])
    from rangekeyutil import with_range_keys
    keyed = Table(with_range_keys(data, [(b"a", b"z", [(100 << 8 | 21, b"", b"value")])]))
    assert keyed.range_dels() is None and keyed.range_keys() is not None
    with pytest.raises(ValueError, match="range keys"):
        compact_tables([keyed], [None], [None])
