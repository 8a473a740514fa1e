"""Range keys in the read path on the device (pebble_amd/csrc/rangekey.hip;
DESIGN.md §3.16): pbl_rangekey_mask against pbl_rangekey_mask_host (which takes
the runs, so that it checks the set builder and the lookup together) and
against the Python statement in rangekeyutil.py, entry for entry;
`Table.range_keys()` and `read(with_range_keys=, mask_suffix=)` end to end."""
import functools
import random

import numpy as np
import pytest
import torch

import rangekeyutil as U
from keyspanutil import assert_same
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, DecodeError, decode as row_decode
from pebble_amd.keyspan import decode as keyspan_decode
from pebble_amd.rangekey import build_set_host, mask, mask_host, to_device
from pebble_amd.rowblk import Writer
from rangekeyutil import ALL, C, D, MAX, SET, T, tr
from scanutil import result_kvs

pytestmark = pytest.mark.gpu

G = U.load_golden()
CASES = U.cases()


def row_block(keys, restart=4):
    w = Writer(restart)
    for k in keys:
        w.add(k, 7 << 8 | 1, b"v")
    return w.finish()


def dev_points(key_blocks):
    """A device batch of point KVs: one row block per list of keys (None: a corrupt block)."""
    blocks = [row_block([b"x"])[:-4] + bytes(4) if ks is None else row_block(ks) for ks in key_blocks]
    return row_decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0))


def dev_runs(runs):
    """The runs decoded on the device from their keyspan blocks, and their to_host() dicts."""
    devs = [keyspan_decode(BlockBatch.from_blocks([U.run_block(r)], "cuda", N.PBL_FMT_ROW, 0), extras=True) for r in runs]
    return devs, [d.to_host() for d in devs]


def check_mask(runs, comparer, key_blocks, t, snapshot=MAX, cover=None, ctx=""):
    """Device mask == host mask over the runs == the Python statement."""
    _, hosts = dev_runs(runs)
    for h, r in zip(hosts, runs):
        assert_same(h, U.run_host(r), ctx)
    batch = dev_points(key_blocks)
    hb = batch.to_host()
    keys = [k for b in range(len(key_blocks)) for k, _, _, _ in result_kvs(hb, b)]
    set_host = build_set_host(hosts, comparer, snapshot)
    set_dev = to_device(set_host, "cuda")
    assert_same(set_dev.to_host(), set_host, ctx)
    cov = None if cover is None else torch.tensor(cover, dtype=torch.int64, device="cuda")
    got = mask(set_dev, batch, comparer, t, cover=cov).cpu().numpy().view(np.uint64).tolist()
    want, st = mask_host(hosts, hb, comparer, t, snapshot, cover)
    assert st == 0 and got == want.tolist(), (ctx, "host")
    good = [k for ks in key_blocks if ks is not None for k in ks]
    assert keys == good
    assert got == U.expected_cover(runs, keys, comparer, t, snapshot, cover), (ctx, "statement")
    return got


def blocks_of(keys, per_block):
    return [keys[i: i + per_block] for i in range(0, len(keys), per_block)] or [[]]


def masking_runs(c):
    return [[(s.encode(), e.encode(), [(tr(10 + i, SET), sfx.encode(), v.encode())])]
            for i, (s, e, sfx, v) in enumerate(c["range_keys"])]


def test_mask_fixtures():
    for c in G["masking"]:
        keys = sorted(p.encode() for p in c["points"])
        got = check_mask(masking_runs(c), T, [keys], c["mask_suffix"].encode(), ctx=c["mask_suffix"])
        assert sorted(k for k, m in zip(keys, got) if m) == sorted(p.encode() for p in c["masked"])


def test_mask_skip_point_example():
    """SkipPoint's comment (range_keys.go:300-340), threshold @7: exactly h@5 and n@4 are masked."""
    runs = [[(b"e", b"m", [(tr(3), b"@9", b"")])], [(b"h", b"q", [(tr(2), b"@6", b"")])], [(b"f", b"l", [(tr(1), b"@3", b"")])]]
    assert check_mask(runs, T, [[b"b@2", b"h@5", b"l@8", b"n@4"]], b"@7") == [0, ALL, 0, ALL]


def test_mask_edges():
    runs = [[(b"c", b"f", [(tr(9), b"", b"nosuffix"), (tr(8), b"@6", b"x"), (tr(7), b"@3", b"y")]),
             (b"h", b"k", [(tr(9), b"", b"only")])]]
    keys = [b"b@1", b"c", b"c@1", b"c@5", b"c@6", b"c@7", b"e@2", b"f@1", b"g@1", b"h@1", b"j@0"]
    assert check_mask(runs, T, [keys], b"@9") == [0, 0, ALL, ALL, 0, 0, ALL, 0, 0, 0, 0]
    assert check_mask(runs, T, [keys], b"@5") == [0, 0, ALL, 0, 0, 0, ALL, 0, 0, 0, 0]
    assert check_mask(runs, T, [keys], b"@2") == [0] * len(keys)   # t above every suffix
    assert check_mask(runs, T, [keys], b"") == [0, 0, ALL, ALL, 0, 0, ALL, 0, 0, 0, 0]
    cover = [5, 0, 7, 0, 9, 0, 0, 11, 0, 0, 13]
    assert check_mask(runs, T, [keys], b"@9", cover=cover) == [5, 0, ALL, ALL, 9, 0, ALL, 11, 0, 0, 13]


@pytest.mark.parametrize("n,per_block", [(1, 1), (63, 63), (64, 64), (65, 65), (65, 7), (257, 100), (1000, 90)])
def test_mask_sizes_and_a_bad_block(n, per_block):
    runs = [U.chain(4, suffix_of=lambda i: b"@%d" % (5 + i)), [(U.gen_key(2), U.gen_key(9), [(tr(500), b"@1", b"w")])]]
    keys = sorted(U.gen_key(i % 11) + b"@%d" % (i // 11) for i in range(n))
    blocks = blocks_of(keys, per_block)
    got = check_mask(runs, T, blocks, b"@9", ctx=(n, per_block))
    assert n < 65 or 0 < sum(1 for x in got if x) < n
    if len(blocks) >= 2:  # KVs of a block that is not OK are untouched
        blocks = blocks[:1] + [None] + blocks[1:]
        check_mask(runs, T, blocks, b"@9", cover=list(range(1, n + 1)), ctx=(n, per_block, "bad block"))


def test_mask_composes_with_a_range_deletion_cover():
    from pebble_amd.rangedel import build_set, cover
    from rangedelutil import run_block as rd_block
    tomb = row_decode(BlockBatch.from_blocks([rd_block([(b"b", 9 << 8 | 15, b"d")])], "cuda", N.PBL_FMT_ROW, 0))
    runs = [[(b"c", b"f", [(tr(3), b"@5", b"x")])]]
    keys = [b"a@1", b"b@1", b"c@1", b"c@7", b"d@1", b"e@9", b"f@1"]
    batch = dev_points([keys])
    cov = cover(build_set([tomb], T), batch, T)
    assert cov.cpu().tolist() == [0, 9, 9, 9, 0, 0, 0]
    _, hosts = dev_runs(runs)
    got = mask(to_device(build_set_host(hosts, T), "cuda"), batch, T, b"@9", cover=cov)
    assert got.data_ptr() == cov.data_ptr() and got.cpu().tolist() == [0, 9, ALL, 9, ALL, 0, 0]


def test_mask_of_a_set_with_a_status_or_none():
    batch = dev_points([[b"a@1", b"b@1"]])
    cov = torch.tensor([3, 4], dtype=torch.int64, device="cuda")
    _, hosts = dev_runs([[(b"a", b"c", [(5 << 8 | 15, b"", b"")])]])
    bad = build_set_host(hosts, T)
    assert bad["blk_status"].tolist() == [N.PBL_UNSUPPORTED]
    assert mask(to_device(bad, "cuda"), batch, T, b"@9", cover=cov).cpu().tolist() == [3, 4]
    empty = build_set_host([], T)
    assert mask(to_device(empty, "cuda"), batch, T, b"@9", cover=cov).cpu().tolist() == [3, 4]
    assert mask(to_device(empty, "cuda"), batch, T, b"@9").cpu().tolist() == [0, 0]


@pytest.mark.parametrize("name,runs,comparer,snapshots", CASES, ids=[c[0] for c in CASES])
def test_mask_cases(name, runs, comparer, snapshots):
    keys = U.points_for(runs, comparer)
    if len(keys) > 400:
        keys = random.Random(1).sample(keys, 400)
        keys.sort(key=functools.cmp_to_key(lambda a, b: U.key_compare(comparer, a, b)))
    if not keys:
        keys = [b"a@1"]
    t = {T: b"@30", C: (20).to_bytes(8, "big") + b"\x09", D: b"s"}[comparer]
    for s in snapshots:
        check_mask(runs, comparer, blocks_of(keys, 64), t, s, ctx=(name, s))


# ---- end to end: a golden columnar table with a pebble.range_key block ---------------------------------
def table_keys(plain):
    keys = []
    for k, _, _, _ in result_kvs(plain.scan([None], [None]).batch.to_host(), 0):
        if not keys or keys[-1] != k:
            keys.append(k)
    return keys


def prefix_of(comparer, k):
    return k[: U.split(comparer, k)]


def table_spans(name, which):
    """Range keys over a golden table's own key prefixes: two different sets of fragmented spans."""
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    data = table_bytes(name)
    plain = Table(data)
    comparer = plain.comparer()
    ps = []
    for k in table_keys(plain):
        p = prefix_of(comparer, k)
        if comparer == C and not p.endswith(b"\x00"):
            continue
        if p and (not ps or ps[-1] != p):
            ps.append(p)
    assert len(ps) >= 8
    n = len(ps)
    # (crdb: walls around the golden table's own, which lie between 2^36 and 2^42)
    sfx = {T: lambda i: b"@%d" % i, C: lambda i: (i << 40).to_bytes(8, "big") + b"\x09", D: lambda i: b"s%d" % i}[comparer]
    if which == 0:
        spans = [(ps[0], ps[2], [(tr(900), sfx(1), b"low"), (tr(800, U.UNSET), sfx(3), b"")]),
                 (ps[2], ps[3], [(tr(900), sfx(1), b"low")]),
                 (ps[n // 2], ps[n // 2 + 2], [(tr(950), sfx(4), b"mid"), (tr(940), b"", b"plain")])]
    else:
        spans = [(ps[1], ps[n // 2 + 1], [(tr(990, U.DEL), b"", b""), (tr(985), sfx(2), b"wide")]),
                 (ps[n - 2], ps[n - 1], [(tr(970), sfx(3), b"tail")])]
    return data, plain, comparer, spans


@pytest.mark.parametrize("name", ["find_val_sep_000011.sst", "cr_schema_000014.sst"])
def test_table_range_keys_and_read(name):
    from pebble_amd.merge import merge_host
    from pebble_amd.sstable import Table
    from pebble_amd.visible import read, visible_host
    from visibleutil import device_result
    data, plain, comparer, spans_a = table_spans(name, 0)
    _, _, _, spans_b = table_spans(name, 1)
    ta, tb = Table(U.with_range_keys(data, spans_a)), Table(U.with_range_keys(data, spans_b))
    assert plain.range_keys() is None and ta.footer.columnar
    assert_same(ta.range_keys().to_host(), U.run_host(spans_a), name)
    assert_same(tb.range_keys().to_host(), U.run_host(spans_b), name)
    runs = [spans_a, spans_b]
    keys = table_keys(plain)
    lo, up = [None, keys[1], keys[len(keys) // 2]], [None, keys[-2], None]
    # a threshold that sorts before every suffix used, so that every range key may mask
    t = {T: b"@9999", C: b"\xff" * 8 + b"\x09", D: b""}[comparer]
    # without the new arguments: the result of the tables without range keys, array for array
    before = device_result(read([plain, plain], lo, up))
    same = device_result(read([ta, tb], lo, up))
    assert_same(same[0], before[0], name, extras=False)
    assert same[1].tolist() == before[1].tolist() and same[2].tolist() == before[2].tolist()
    union = merge_host([x.scan(lo, up).batch.to_host() for x in (ta, tb)], comparer=comparer)
    ukeys = [k for b in range(len(lo)) for k, _, _, _ in result_kvs(union[0], b)]
    for snapshot in (MAX, 960):
        points, rk = read([ta, tb], lo, up, snapshot=snapshot, with_range_keys=True, mask_suffix=t)
        spans = U.expected_spans(runs, comparer, snapshot)
        assert_same(rk.to_host(), U.layout([U.clip_spans(spans, a, b, comparer) for a, b in zip(lo, up)]), (name, snapshot))
        cov = U.expected_cover(runs, ukeys, comparer, t, snapshot)
        if name.startswith("cr_schema"):  # (the other table's keys have no versions: nothing to mask)
            assert any(cov) and not all(cov)
        want = visible_host(union[0], comparer=comparer, snapshot=snapshot, cover=np.array(cov, np.uint64))
        got = device_result(points)
        assert_same(got[0], want[0], (name, snapshot), extras=False)
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), snapshot
    # the mask alone, and the range keys alone
    only = device_result(read([ta, tb], lo, up, mask_suffix=t))
    assert_same(only[0], visible_host(union[0], comparer=comparer,
                                      cover=np.array(U.expected_cover(runs, ukeys, comparer, t), np.uint64))[0], name,
                extras=False)
    pts, rk = read([ta, tb], lo, up, with_range_keys=True)
    assert_same(device_result(pts)[0], before[0], name, extras=False)
    assert rk.batch.n_blocks == 3


def test_row_table_range_keys_are_out_of_scope():
    from pebble_amd.sstable import RANGE_KEY_NAME, Table
    from tableutil import table_bytes
    row = Table(table_bytes("h_no_compression.sst"))
    assert not row.footer.columnar and row.range_keys() is None
    row.metaindex()[RANGE_KEY_NAME] = (0, 0)
    with pytest.raises(DecodeError, match="out of scope"):
        row.range_keys()
