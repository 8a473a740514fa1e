"""Columnar keyspan blocks on the device (pebble_amd/csrc/keyspan.hip; DESIGN.md
§3.15).  Every device result is compared, byte for byte on every array and
total, with the Python decoder of tests/keyspanutil.py and with the host form
(pbl_keyspan_decode_host); then the run is compared with the row path over the
same tombstones, and `Table.range_dels()` / `read()` are checked over golden
columnar tables re-emitted with a keyspan block of range deletions."""
import random

import numpy as np
import pytest

from keyspanutil import (BOUNDS, HEADER, RANGEDEL, assert_same, assert_same_sizes, block_of_spans, decode_block, expected, gap_blocks,
                         load_golden, random_spans, rangedel_spans, sized, with_range_dels)
from mergeutil import C, D, T
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, Capacity, DecodeError, decode as row_decode
from pebble_amd.keyspan import decode, decode_host, encode_block, size
from scanutil import ARRAYS, TOTALS, result_kvs

pytestmark = pytest.mark.gpu

G = load_golden()
MAX56 = (1 << 56) - 1


def batch_of(blocks, ssn=0):
    bb = BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_COL_DEFAULT, 0)  # (the format is not read)
    bb.synthetic_seq_num = ssn
    return bb


def check(blocks, ssn=0, ctx=""):
    """Device == Python decoder == host form, with the extras; without them the
    run alone is the same.  Returns the expected result."""
    want = expected(blocks, ssn)
    got = decode(batch_of(blocks, ssn), extras=True).to_host()
    assert_same(got, want, (ctx, "device"))
    assert_same(decode_host(blocks, extras=True, synthetic_seq_num=ssn), want, (ctx, "host"))
    plain = decode(batch_of(blocks, ssn)).to_host()
    assert_same(plain, want, (ctx, "no extras"), extras=False)
    return want


def assert_same_batch(a, b, ctx=""):
    """Two batches in to_host()'s layout: every array and total, exactly."""
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k, x[:8], y[:8])
    for k in TOTALS:
        assert int(a[k]) == int(b[k]), (ctx, k, a[k], b[k])


def rd(n, seq=lambda i: 1000 - i):
    """n RANGEDEL keys with descending sequence numbers."""
    return [(seq(i) << 8 | RANGEDEL, b"", b"") for i in range(n)]


def key(i, n=8):
    return b"%0*d" % (n, i)


# ---- 1. the reference's blocks --------------------------------------------------------------------
def test_golden_blocks():
    blocks = [bytes.fromhex(b["hex"]) for b in G["blocks"]]
    for b, blk in zip(G["blocks"], blocks):
        want = check([blk], 0, b["name"])
        assert want["n_kv"] == sum(len(s["keys"]) for s in b["spans"]) and want["status_mask"] == 0
        for w in b["walks"]:
            check([blk], w["synthetic_seq_num"], (b["name"], "walk"))
    check(blocks, 0, "all")
    check(blocks, 99, "all, synthetic")


# ---- 2. shapes ------------------------------------------------------------------------------------
def test_smallest_blocks():
    one = block_of_spans([(b"a", b"b", rd(1))])
    assert int.from_bytes(one[:4], "little") == 2 and int.from_bytes(one[7:11], "little") == 1
    assert check([one])["n_kv"] == 1
    empty = block_of_spans([])
    single = encode_block([b"a"], [0], [5 << 8 | RANGEDEL], [b""], [b""])
    for blk in (empty, single):
        want = check([blk])
        assert want["n_kv"] == 0 and want["status_mask"] == 0
    check([empty, one, single, one])


@pytest.mark.parametrize("n", [65, 257])
def test_one_wide_span(n):
    """One span whose keys cross a wave's and a tile's edge; with a neighbour on each side."""
    want = check([block_of_spans([(b"a", b"b", rd(2)), (b"b", b"cc", rd(n)), (b"cc", b"d", rd(1))])])
    assert want["n_kv"] == n + 3


def test_many_spans():
    """600 spans: more than one span tile, gaps among them, range keys."""
    rng = random.Random(600)
    want = check([block_of_spans(random_spans(rng, 600))])
    assert want["n_kv"] >= 600 and len(set(want["span"].tolist())) == 600
    check([block_of_spans(random_spans(rng, 300, range_keys=False)), block_of_spans(random_spans(rng, 600, max_keys=1))])


@pytest.mark.parametrize("case", gap_blocks(), ids=[c[0] for c in gap_blocks()])
def test_gaps_and_their_corruptions(case):
    name, blk, status = case
    want = check([blk], 0, name)
    assert int(want["blk_status"][0]) == status


UINT_FORMS = [(1, False), (1, True), (2, False), (2, True), (4, False), (4, True), (8, False), (0, False), (0, True)]


@pytest.mark.parametrize("w,delta", UINT_FORMS, ids=["%db%s" % (w, "+delta" if d else "") for w, d in UINT_FORMS])
def test_uint_widths(w, delta):
    """idx[] and the trailers at every width, with and without a delta base; the
    constant form (width 0): legal for trailers, an idx[] without keys."""
    n = 70
    bounds = [key(i) for i in range(n + 1)]
    step = {0: 0, 1: 1, 2: 256, 4: 1 << 20, 8: 1 << 33}[w]
    # trailers in column 2 at (w, delta), idx as the writer picks it; with a delta
    # base or 8 bytes the first sequence number is 2^56 - 1
    top = MAX56 << 8 | RANGEDEL if delta or w == 8 else (n - 1) * step + (RANGEDEL if w else 0)
    trailers = [top - i * step for i in range(n)]
    blk = encode_block(bounds, list(range(n + 1)), trailers, [b""] * n, [b""] * n, {2: (w, delta)})
    want = check([blk], 0, "trailers")
    assert want["n_kv"] == n and want["trailer"].tolist() == trailers
    # idx in column 1 at (w, delta): the first boundary's index is the base
    i0 = 3 if delta else 0
    istep = {0: 0, 1: 1, 2: 300, 4: 400, 8: 500}[w]
    idx = [i0 + i * istep for i in range(4)]
    rows = idx[-1] + 2
    blk = encode_block(bounds[:4], idx, [(rows - i) << 8 | RANGEDEL for i in range(rows)], [b""] * rows, [b""] * rows,
                       {1: (w, delta)})
    want = check([blk], 0, "idx")
    assert (int(want["blk_status"][0]), want["n_kv"]) == ((BOUNDS, 0) if w == 0 else (0, 3 * istep))


def test_offset_widths_and_key_lengths():
    """Boundary offsets at widths 1, 2 and 4 (past 255 B and past 64 KiB of
    boundary data), the suffix and value columns in the zero encoding, a boundary
    key of 0 bytes, one of 300 bytes and one of 700 (past the 512 bytes that 8
    lanes copy)."""
    small = block_of_spans([(b"", b"a", rd(2)), (b"a", b"b" * 300, rd(1)), (b"b" * 300, b"c", rd(3)),
                            (b"c", b"d" * 700, rd(2)), (b"d" * 700, b"e", rd(1))])
    wide = block_of_spans([(key(i, 300), key(i + 1, 300), rd(1 + i % 2)) for i in range(240)])
    narrow = block_of_spans([(key(i, 3), key(i + 1, 3), rd(1)) for i in range(40)])
    for blk, w in ((narrow, 1), (small, 2), (wide, 4)):
        at = int.from_bytes(blk[12:16], "little")
        assert blk[at] == w  # the boundary offsets' encoding byte
        s3, s4 = int.from_bytes(blk[27:31], "little"), int.from_bytes(blk[32:36], "little")
        assert blk[s3] == 0 and blk[s4] == 0  # suffixes and values: the zero encoding
    want = check([small, wide, narrow])
    assert want["status_mask"] == 0 and want["key_bytes_total"] > 65536 + 600
    kvs = result_kvs(want, 0)
    assert kvs[0][0] == b"" and kvs[2][2] == b"b" * 300 and kvs[3][0] == b"b" * 300


def test_truncated_blocks():
    """A block cut after the header, after each column's start, and without the padding byte."""
    rng = random.Random(3)
    good = block_of_spans(random_spans(rng, 30))
    starts = [int.from_bytes(good[12 + 5 * c: 16 + 5 * c], "little") for c in range(5)]
    cuts = [0, 3, 4, 10, 11, 12, 35, 36] + starts + [s + 1 for s in starts] + [len(good) - 1]
    for cut in cuts:
        blk = good[:cut]
        want = check([good, blk, good], 0, cut)
        assert want["blk_status"].tolist() == [0, HEADER, 0], cut


@pytest.mark.parametrize("nb", [1, 3, 17])
def test_batches_with_a_corrupt_block(nb):
    rng = random.Random(nb)
    blocks = [block_of_spans(random_spans(rng, rng.randrange(1, 80))) for _ in range(nb)]
    whole = expected(blocks)
    bad = bytearray(blocks[nb // 2])
    bad[5] = 4  # four columns
    blocks[nb // 2] = bytes(bad)
    want = check(blocks, 0, nb)
    assert int(want["blk_status"][nb // 2]) == HEADER and want["n_bad_blocks"] == 1
    for q in range(nb):
        if q != nb // 2:
            assert result_kvs(want, q) == result_kvs(whole, q)


def test_more_blocks_than_one_chunk_of_the_block_scan():
    """300 small blocks: the scan over blocks takes two chunks of 256."""
    rng = random.Random(300)
    blocks = [block_of_spans(random_spans(rng, rng.randrange(0, 4))) for _ in range(300)]
    blocks[257] = blocks[257][:20]
    want = check(blocks, 0, "300 blocks")
    assert want["n_bad_blocks"] == 1 and int(want["blk_status"][257]) == HEADER and want["n_kv"] > 300


def test_capacities_and_the_size_call():
    rng = random.Random(9)
    blocks = [block_of_spans(random_spans(rng, 50)), block_of_spans(random_spans(rng, 7))]
    want = expected(blocks)
    sz = size(batch_of(blocks), extras=True)
    assert (sz["n_kv"], sz["key_bytes"], sz["val_bytes"], sz["suffix_bytes"], sz["value_bytes"], sz["status_mask"]) == \
        (want["n_kv"], want["key_bytes_total"], want["val_bytes_total"], len(want["suffix_bytes"]),
         len(want["value_bytes"]), 0)
    assert sz["blk_status"].tolist() == [0, 0]
    full = Capacity(want["n_kv"], want["key_bytes_total"], want["val_bytes_total"], 0)
    ecap = (len(want["suffix_bytes"]), len(want["value_bytes"]))
    assert_same(decode(batch_of(blocks), extras=True, cap=full, extra_cap=ecap).to_host(), want, "exact")
    shorts = [(Capacity(full.kv - 1, full.key, full.val, 0), ecap), (Capacity(full.kv, full.key - 1, full.val, 0), ecap),
              (Capacity(full.kv, full.key, full.val - 1, 0), ecap), (full, (ecap[0] - 1, ecap[1])),
              (full, (ecap[0], ecap[1] - 1))]
    for cap, ec in shorts:
        # (that no byte is written: test_overflow_leaves_the_arrays_alone)
        res = decode(batch_of(blocks), extras=True, cap=cap, extra_cap=ec)
        assert_same_sizes(res.to_host(), sized(want), (cap, ec))
        assert_same(decode_host(blocks, extras=True, cap=cap, extra_cap=ec), sized(want), (cap, ec, "host"))
    d = decode(batch_of(blocks), cap=Capacity(full.kv - 1, full.key, full.val, 0))
    assert d.read_totals().status_mask == 1 << N.PBL_OVERFLOW and d.read_totals().n_kv == want["n_kv"]


def test_overflow_leaves_the_arrays_alone():
    import torch
    blocks = [block_of_spans(random_spans(random.Random(4), 40))]
    want = expected(blocks)
    from pebble_amd.batch import DecodedBatch
    from pebble_amd import keyspan as K
    bb = batch_of(blocks)
    tb = K.total_boundaries(bb)
    assert tb == int.from_bytes(blocks[0][:4], "little")
    cap = Capacity(want["n_kv"], want["key_bytes_total"] - 1, want["val_bytes_total"], 0)
    out = DecodedBatch.allocate(1, cap, "cuda", entry_off=True, restarts=False)
    for t in (out.trailer, out.key_off, out.val_off, out.key_bytes, out.val_bytes, out.entry_off, out.kv_flags):
        t.fill_(0x5A if t.dtype == torch.uint8 else 0x5A5A5A5A)
    ws = K._workspace(bb, tb, torch.cuda.current_stream())
    K._run(bb, out, None, ws, tb, torch.cuda.current_stream(), False)
    torch.cuda.synchronize()
    assert out.read_totals().status_mask == 1 << N.PBL_OVERFLOW
    assert bool((out.key_bytes == 0x5A).all()) and bool((out.val_bytes == 0x5A).all())
    assert bool((out.trailer == 0x5A5A5A5A).all()) and bool((out.key_off == 0x5A5A5A5A).all())


def test_too_small_a_workspace_is_reported_per_block():
    """total_boundaries below the blocks' own: the blocks that do not fit are
    PBL_INVALID_ARG, the others decode."""
    import torch
    from pebble_amd import keyspan as K
    from pebble_amd.batch import DecodedBatch
    rng = random.Random(12)
    blocks = [block_of_spans(random_spans(rng, 10)), block_of_spans(random_spans(rng, 300))]
    bb = batch_of(blocks)
    tb = int.from_bytes(blocks[0][:4], "little") + 5
    want = expected(blocks[:1])
    out = DecodedBatch.allocate(2, Capacity(want["n_kv"], want["key_bytes_total"], want["val_bytes_total"], 0), "cuda",
                                entry_off=True, restarts=False)
    st = torch.cuda.current_stream()
    K._run(bb, out, None, K._workspace(bb, tb, st), tb, st, False)
    torch.cuda.synchronize()
    h = out.to_host()
    assert h["blk_status"].tolist() == [0, N.PBL_INVALID_ARG] and result_kvs(h, 0) == result_kvs(want, 0)


# ---- 3. the same tombstones through the row path ------------------------------------------------------
@pytest.mark.parametrize("comparer", [D, T, C], ids=["default", "testkeys", "crdb"])
@pytest.mark.parametrize("shape", ["distinct", "same_start", "shared"])
def test_equivalence_with_the_row_path(comparer, shape):
    from pebble_amd.rangedel import build_set
    from rangedelutil import random_runs, run_block
    rng = random.Random(10 * comparer + len(shape))
    runs = random_runs(rng, 3, 70, comparer, shape=shape)
    row = [row_decode(BlockBatch.from_blocks([run_block(kvs)], "cuda", N.PBL_FMT_ROW, 0)) for kvs in runs]
    col = [decode(batch_of([block_of_spans(rangedel_spans(kvs))])) for kvs in runs]
    for r, c, kvs in zip(row, col, runs):
        a, b = result_kvs(r.to_host(), 0), result_kvs(c.to_host(), 0)
        assert [x[:3] for x in a] == [x[:3] for x in b] == [(s, t, e) for s, t, e in kvs]
    for snapshot in ((1 << 56) - 1, 500):
        sa, sb = build_set(row, comparer, snapshot).to_host(), build_set(col, comparer, snapshot).to_host()
        assert sa["status_mask"] == 0 and sa["n_kv"] > 0
        assert_same_batch(sa, sb, snapshot)


# ---- 4. tables and read() -----------------------------------------------------------------------------
def table_with_tombstones(name, seq):
    """(the golden table, the table re-emitted with range deletions over its own
    keys, the run's KVs)."""
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    data = table_bytes(name)
    plain = Table(data)
    keys = []
    for k, _, _, _ in result_kvs(plain.scan([None], [None]).batch.to_host(), 0):
        if not keys or keys[-1] != k:
            keys.append(k)
    assert len(keys) >= 12
    n = len(keys)
    cuts = [(1, 3, [seq + 2, seq]), (3, 4, [seq + 1]), (n // 2, n // 2 + 3, [seq + 3]), (n - 3, n - 1, [seq + 5, seq + 4, 1])]
    spans = [(keys[a], keys[b], [(s << 8 | RANGEDEL, b"", b"") for s in seqs]) for a, b, seqs in cuts]
    kvs = [(s, t, e) for s, e, ks in spans for t, _, _ in ks]
    return plain, Table(with_range_dels(data, spans)), kvs


@pytest.mark.parametrize("name", ["find_val_sep_000011.sst", "cr_schema_000014.sst"])
def test_columnar_table_with_range_deletions(name):
    from pebble_amd.merge import merge_host
    from pebble_amd.rangedel import cover_host
    from pebble_amd.visible import read, visible_host
    from rangedelutil import run_host
    from visibleutil import MAX, device_result
    plain, table, kvs = table_with_tombstones(name, 100)
    assert plain.range_dels() is None and table.footer.columnar
    run = table.range_dels()
    assert [x[:3] for x in result_kvs(run.to_host(), 0)] == kvs
    comparer = table.comparer()
    lo, up = [None, kvs[0][0]], [None, kvs[-1][2]]
    before = device_result(read([plain], lo, up))
    union = merge_host([table.scan(lo, up).batch.to_host()], comparer=comparer)
    for snapshot in (MAX, 103):
        got = device_result(read([table], lo, up, snapshot=snapshot))
        cov, st = cover_host([run_host(kvs)], union[0], comparer, snapshot)
        assert st == 0 and cov.any()
        want = visible_host(union[0], comparer=comparer, snapshot=snapshot, cover=cov)
        assert_same_batch(got[0], want[0], snapshot)
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), snapshot
    got = device_result(read([table], lo, up))
    assert 0 < got[0]["n_kv"] < before[0]["n_kv"]


def test_read_over_a_columnar_and_a_row_table():
    from pebble_amd.merge import merge_host
    from pebble_amd.rangedel import cover_host
    from pebble_amd.sstable import Table
    from pebble_amd.visible import read, visible_host
    from rangedelutil import run_host
    from tableutil import table_bytes
    from visibleutil import MAX, device_result
    _, table, kvs = table_with_tombstones("find_val_sep_000011.sst", 100)
    row = Table(table_bytes("h_no_compression.sst"))
    tables = [table, row]
    comparer = table.comparer()
    assert comparer == row.comparer()
    lo, up = [None, b"g"], [None, b"h"]
    hosts = [run_host(kvs), row.range_dels().to_host()]
    union = merge_host([t.scan(lo, up).batch.to_host() for t in tables], comparer=comparer)
    for levels in (None, [0, 1], [1, 0]):
        got = device_result(read(tables, lo, up, levels=levels))
        if levels is None:
            cov, st = cover_host(hosts, union[0], comparer, MAX)
        else:
            cov, st = cover_host(hosts, union[0], comparer, MAX, levels=levels, src_run=union[1], run_levels=levels)
        assert st == 0 and cov.any()
        want = visible_host(union[0], comparer=comparer, cover=cov)
        assert_same_batch(got[0], want[0], levels)
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), levels


def test_a_corrupt_keyspan_block_in_a_table_raises():
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    bad = encode_block([b"a", b"b", b"c"], [1, 0, 2], [5 << 8 | RANGEDEL] * 2, [b""] * 2, [b""] * 2)  # idx[] decreasing
    assert decode_block(bad)[0] == BOUNDS
    with pytest.raises(DecodeError):
        Table(with_range_dels(table_bytes("find_val_sep_000011.sst"), [], block=bad)).range_dels()
