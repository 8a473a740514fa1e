"""Range deletions in the read path on the device (pebble_amd/csrc/rangedel.hip,
the view's _rd entry points).  Every device result is compared
with the host functions on every array: the set with pbl_rangedel_set_host, the
cover with pbl_rangedel_cover_host (which takes the runs, so that it checks the
builder and the lookup together), the view with pbl_visible_batch_host_rd."""
import random

import numpy as np
import pytest

from mergeutil import BAD, C, D, T
from pebble_amd import _native as N
from pebble_amd.rangedel import build_set, build_set_host, cover, cover_host
from pebble_amd.rowblk import Writer, make_trailer
from pebble_amd.visible import read, visible, visible_host
from rangedelutil import (RANGEDEL, assert_visible_rd_is, expected_set, expected_visible_rd, gen_key, golden_sections,
                          load_golden, random_runs, replay_case, run_block, run_kvs, section_levels, set_kvs)
from scanutil import ARRAYS, TOTALS, result_kvs
from visibleutil import MAX, assert_same, cases, device_result, one_key_block, tr

pytestmark = pytest.mark.gpu

G = load_golden()


def dev_decode(blocks):
    from pebble_amd.batch import BlockBatch, decode
    return decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0))


def row_block(kvs, restart=4):
    w = Writer(restart)
    for kv in kvs:
        w.add(kv[0], kv[1], kv[2])
    return w.finish()


def corrupt(block: bytes) -> bytes:
    return block[:-4] + bytes(4)  # zero restarts: PBL_CORRUPT_NO_RESTARTS


def dev_run(kvs):
    """A run: the row-format range-del block (restart interval 1), decoded on the device."""
    return dev_decode([corrupt(run_block([(b"x", 1 << 8 | 15, b"y")])) if kvs is None else run_block(kvs)])


def assert_same_batch(a, b, ctx=""):
    """Two batches in to_host()'s layout: every array and total, exactly."""
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x.astype(np.uint64) == y.astype(np.uint64)).all(), (ctx, k, x[:8], y[:8])
    for k in TOTALS:
        assert int(a[k]) == int(b[k]), (ctx, k, a[k], b[k])


def check_set(runs, comparer, snapshots=(MAX,), ctx=""):
    devs = [dev_run(kvs) for kvs in runs]
    hosts = [d.to_host() for d in devs]
    for s in snapshots:
        got = build_set(devs, comparer, s).to_host()
        assert_same_batch(got, build_set_host(hosts, comparer, s), (ctx, s))
    return devs, hosts, got


# ---- 1. the set builder ---------------------------------------------------------------------------
SET_PARAMS = [(n_runs, per_run, shape) for n_runs in (1, 16) for per_run in (1, 63, 64, 65, 300)
              for shape in ("distinct", "same_start", "shared")]


@pytest.mark.parametrize("n_runs,per_run,shape", SET_PARAMS, ids=["%dx%d-%s" % p for p in SET_PARAMS])
def test_set_builder(n_runs, per_run, shape):
    rng = random.Random(100 * n_runs + per_run)
    runs = random_runs(rng, n_runs, per_run, D, shape=shape)
    _, _, got = check_set(runs, D, (MAX, 500), (n_runs, per_run, shape))
    assert got["status_mask"] == 0 and got["n_kv"] > 0
    if n_runs * per_run <= 300:  # the third statement, where Python's brute force is quick
        assert set_kvs(got) == expected_set(runs, D, 500)
    if shape == "distinct":
        assert got["n_kv"] == 2 * n_runs * per_run
    if shape == "same_start":
        assert got["n_kv"] == 1 + n_runs
    if shape == "shared":
        assert any(k == gen_key(5000) for k, _ in set_kvs(got))


@pytest.mark.parametrize("keylen,n_runs,per_run", [(1, 1, 100), (1, 16, 7), (300, 1, 65), (300, 16, 65)])
def test_set_builder_key_lengths(keylen, n_runs, per_run):
    runs = random_runs(random.Random(keylen), n_runs, per_run, D, keylen=keylen)
    _, _, got = check_set(runs, D, (MAX,), keylen)
    assert got["n_kv"] == 2 * n_runs * per_run and got["key_bytes_total"] == keylen * got["n_kv"]


@pytest.mark.parametrize("comparer", [T, C])
def test_set_builder_comparers(comparer):
    for shape in ("distinct", "shared"):
        runs = random_runs(random.Random(comparer), 5, 40, comparer, shape=shape)
        _, _, got = check_set(runs, comparer, (MAX, 300), (comparer, shape))
        assert set_kvs(got) == expected_set(runs, comparer, 300)


def test_set_statuses_and_empty_runs():
    rd = lambda s, e, t: (s, make_trailer(t, RANGEDEL), e)  # noqa: E731
    good = [rd(b"a", b"b", 5), rd(b"c", b"d", 5)]
    kind = [(b"a", make_trailer(5, 1), b"b")]
    unsorted = [rd(b"c", b"d", 5), rd(b"a", b"b", 5)]
    overlap = [rd(b"a", b"c", 5), rd(b"b", b"d", 5)]
    inverted = [rd(b"b", b"a", 5)]
    U, A = N.PBL_UNSUPPORTED, N.PBL_INVALID_ARG
    for runs, st in (([good, None], BAD), ([kind, good], U), ([good, unsorted], A), ([overlap], A), ([inverted], A),
                     ([unsorted, kind, None], BAD), ([unsorted, kind], U), ([[], good, []], 0), ([[]], 0)):
        _, _, got = check_set(runs, D, (MAX,), st)
        assert got["blk_status"].tolist() == [st] and (st == 0 or got["n_kv"] == 0)
    # a set with a status covers nothing
    devs = [dev_run(overlap)]
    batch = dev_decode([row_block([(b"a", tr(1), b"v"), (b"b", tr(1), b"v")])])
    s = build_set(devs, D)
    assert s.read_totals().status_mask == 1 << A
    assert cover(s, batch, D).cpu().tolist() == [0, 0]


# ---- 2. the cover lookup --------------------------------------------------------------------------
def lookup_runs():
    """260 fragments [100 f, 100 f + 50) dealt to 4 runs."""
    rng = random.Random(5)
    frags = [(gen_key(100 * f), make_trailer(rng.randrange(1, 1000), RANGEDEL), gen_key(100 * f + 50)) for f in range(260)]
    return [frags[r::4] for r in range(4)]


@pytest.fixture(scope="module")
def lookup():
    runs = lookup_runs()
    devs = [dev_run(kvs) for kvs in runs]
    return runs, devs, [d.to_host() for d in devs]


@pytest.mark.parametrize("n,nb", [(n, nb) for n in (1, 255, 256, 257, 70000) for nb in (1, 300)])
def test_cover_lookup(lookup, n, nb):
    runs, devs, hosts = lookup
    # a key before the first boundary, then keys on and between the boundaries and past the last one
    step = 1 if n == 70000 else max(1, 26100 // n)
    keys = [b"!"] + [gen_key(i * step) for i in range(n - 1)]
    per = -(-n // nb)
    blocks = [row_block([(k, tr(7), b"") for k in keys[q * per:(q + 1) * per]], 16) for q in range(nb)]
    batch = dev_decode(blocks)
    h = batch.to_host()
    assert h["n_kv"] == n and h["status_mask"] == 0
    for snapshot in (500, MAX):
        s = build_set(devs, D, snapshot)
        got = cover(s, batch, D).cpu().numpy().view(np.uint64)
        want, st = cover_host(hosts, h, D, snapshot)
        assert st == 0 and got.tolist() == want.tolist(), (n, nb, snapshot)
    assert got[0] == 0 and (n < 70000 or (got[26051:] == 0).all() and got[1:26000:100].all())
    # the empty set
    empty = build_set([dev_run([])], D)
    assert empty.read_totals().n_kv == 0 and not cover(empty, batch, D).cpu().numpy().any()


def test_cover_skips_bad_blocks(lookup):
    runs, devs, hosts = lookup
    blocks = [row_block([(gen_key(10), tr(7), b"")]), corrupt(row_block([(b"x", tr(1), b"")])), row_block([(gen_key(120), tr(7), b"")])]
    batch = dev_decode(blocks)
    h = batch.to_host()
    got = cover(build_set(devs, D), batch, D).cpu().numpy().view(np.uint64)
    want, _ = cover_host(hosts, h, D)
    assert got.tolist() == want.tolist() and got[0] > 0 and len(got) == 2


# ---- 3. the view with a cover ---------------------------------------------------------------------
def dev_batch(blocks, restart=4):
    import torch
    d = dev_decode([corrupt(row_block([(b"x", 1 << 8 | 1, b"")])) if b is None else row_block(b, restart) for b in blocks])
    extra = [kv[3] if len(kv) > 3 else 0 for b in blocks for kv in (b or [])]
    if any(extra):
        d.kv_flags[: len(extra)] |= torch.tensor(extra, dtype=torch.uint8, device="cuda")
    return d


def random_tombstones(rng, blocks, comparer, n=12):
    """Unfragmented tombstones over the case's own keys and sequence numbers."""
    from pebble_amd.blockiter import key_compare
    import functools
    keys = sorted({kv[0] for b in blocks for kv in (b or [])}, key=functools.cmp_to_key(lambda a, b: key_compare(comparer, a, b)))
    seqs = sorted({kv[1] >> 8 for b in blocks for kv in (b or [])})
    out = []
    for _ in range(n if len(keys) > 1 else 0):
        i, j = sorted(rng.sample(range(len(keys)), 2))
        if key_compare(comparer, keys[i], keys[j]) < 0:
            out.append((keys[i], keys[j] + (b"" if rng.random() < 0.5 or comparer != D else b"\x00"), rng.choice(seqs) + rng.randrange(2)))
    return out


CASES = [c for c in cases() if c[2]]


@pytest.mark.parametrize("name,comparer,blocks,snaps", CASES, ids=[c[0] for c in CASES])
def test_view_with_a_cover(name, comparer, blocks, snaps):
    rng = random.Random(len(name))
    tombs = random_tombstones(rng, blocks, comparer)
    runs = [run_kvs(tombs[r::3], comparer) for r in range(3)]
    devs = [dev_run(kvs) for kvs in runs]
    hosts = [d.to_host() for d in devs]
    d = dev_batch(blocks)
    h = d.to_host()
    seqs = sorted({t for _, _, t in tombs}) or [1]
    for snapshot in sorted(set(snaps) | {seqs[0], seqs[len(seqs) // 2] + 1}):
        s = build_set(devs, comparer, snapshot)
        cov = cover(s, d, comparer)
        cov_h, st = cover_host(hosts, h, comparer, snapshot)
        assert st == 0 and cov.cpu().numpy().view(np.uint64).tolist() == cov_h.tolist(), (name, snapshot)
        for keep in (False, True):
            r = device_result(visible(d, comparer=comparer, snapshot=snapshot, keep_operands=keep, cover=cov))
            assert_same(r, visible_host(h, comparer=comparer, snapshot=snapshot, keep_operands=keep, cover=cov_h), (name, snapshot, keep))
            if snapshot == MAX:
                assert_visible_rd_is(r, expected_visible_rd(h, comparer, snapshot, keep, cov_h), (name, keep))
    # no cover: the entry points without range deletions, byte for byte
    assert_same(device_result(visible(d, comparer=comparer, cover=None)), device_result(visible(d, comparer=comparer)), name)
    import torch
    zero = torch.zeros(max(h["n_kv"], 1), dtype=torch.int64, device="cuda")
    assert_same(device_result(visible(d, comparer=comparer, cover=zero)), device_result(visible(d, comparer=comparer)), name)


def test_one_key_block_half_covered():
    """One group longer than any tile, its older half under a tombstone."""
    d = dev_batch([one_key_block()], restart=16)
    h = d.to_host()
    devs = [dev_run([(b"the key", make_trailer(35001, RANGEDEL), b"the key\x00")])]
    hosts = [x.to_host() for x in devs]
    s = build_set(devs, D)
    cov = cover(s, d, D)
    cov_h, _ = cover_host(hosts, h, D)
    assert cov.cpu().tolist() == cov_h.tolist() == [35001] * 70000
    for keep in (False, True):
        r = device_result(visible(d, comparer=D, keep_operands=keep, cover=cov))
        assert_same(r, visible_host(h, comparer=D, keep_operands=keep, cover=cov_h), keep)
    (k, t, v, f), = result_kvs(visible(d, comparer=D, cover=cov).batch.to_host(), 0)
    assert (k, t >> 8) == (b"the key", 70000) and v == bytes(x % 251 for x in range(35001, 70001))


@pytest.mark.parametrize("di", range(len(G["defines"])))
def test_golden_range_del_cases_on_the_device(di):
    """The kept cases of testdata/range_del end to end on the device: decode,
    merge, set, cover, view, with the sections' levels (define 3 needs them:
    tests/test_rangedel.py::test_golden_range_del_cases)."""
    from pebble_amd.merge import merge
    d = G["defines"][di]
    secs = golden_sections(d, G["kinds"])
    lv = section_levels(d)
    points = [dev_decode([row_block(pts)]) for pts, _, _ in secs]
    runs = [dev_run(kvs) for _, kvs, _ in secs]
    hosts = [r.to_host() for r in runs]
    m = merge(points, comparer=D)
    merged, mh = m.batch, m.batch.to_host()
    wrong = []
    for c in d["cases"]:
        s = build_set(runs, D, c["seq"], levels=lv)
        assert s.read_totals().status_mask == 0
        assert_same_batch(s.to_host(), build_set_host(hosts, D, c["seq"], levels=lv), (di, c["seq"]))
        assert s.to_host()["entry_off"].tolist() == build_set_host(hosts, D, c["seq"], levels=lv)["entry_off"].tolist()
        cov = cover(s, merged, D, src_run=m.src_run, run_levels=lv)
        want, _ = cover_host(hosts, mh, D, c["seq"], levels=lv, src_run=m.src_run.cpu().numpy(), run_levels=lv)
        assert cov.cpu().numpy().view(np.uint64).tolist() == want.tolist(), (di, c["seq"])
        r = visible(merged, comparer=D, snapshot=c["seq"], cover=cov).batch.to_host()
        assert r["status_mask"] == 0
        got = replay_case([(k, v) for k, _, v, _ in result_kvs(r, 0)], c)
        wrong += [(c["op"], c["seq"], i, g, e) for i, (g, e) in enumerate(zip(got, c["expected"])) if g != e]
    print("define", di, len(d["cases"]), "cases,", len(wrong), "lines differ", wrong)
    assert not wrong, (di, wrong)


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_leveled_cover(lookup, n):
    """Random levels for the runs and for the KVs' sources: device against host."""
    import torch
    runs, devs, hosts = lookup
    rng = random.Random(n)
    keys = [gen_key(i * max(1, 26100 // n)) for i in range(n)]
    batch = dev_decode([row_block([(k, tr(500), b"") for k in keys[q::3]], 16) for q in range(3)])
    h = batch.to_host()
    for levels, run_levels in (([0, 1, 2, 3], [2, 0, 3, 1]), ([5, 5, 0, 9], [5, 6, 0, 1] + [7] * 12)):
        src = np.array([rng.randrange(len(run_levels)) for _ in range(n)], np.uint8)
        s = build_set(devs, D, 600, levels=levels)
        sh = build_set_host(hosts, D, 600, levels=levels)
        assert_same_batch(s.to_host(), sh, levels)
        assert s.to_host()["entry_off"].tolist() == sh["entry_off"].tolist() and sh["entry_off"].any()
        got = cover(s, batch, D, src_run=torch.from_numpy(src).cuda(), run_levels=run_levels).cpu().numpy().view(np.uint64)
        want, st = cover_host(hosts, h, D, 600, levels=levels, src_run=src, run_levels=run_levels)
        assert st == 0 and got.tolist() == want.tolist()
        assert n == 1 or ((got == N.PBL_RANGEDEL_ALL).any() and ((got > 0) & (got < N.PBL_RANGEDEL_ALL)).any())
        # a set built with levels, looked up without them: the sequence-number rule
        plain = cover(s, batch, D).cpu().numpy().view(np.uint64)
        assert plain.tolist() == cover_host(hosts, h, D, 600)[0].tolist()


# ---- 4. read() and the tables ---------------------------------------------------------------------
def test_read_with_caller_supplied_runs():
    from pebble_amd.merge import merge_host
    from pebble_amd.sstable import Table
    from tableutil import table_bytes
    tables = [Table(table_bytes("h_no_compression.sst")), Table(table_bytes("h_two_level.sst"))]
    comparer = tables[0].comparer()
    lo, up = [None, b"b", b"m"], [None, b"d", b"m\x00"]
    scans = [t.scan(lo, up).batch.to_host() for t in tables]
    keys = sorted({k for k, _, _, _ in result_kvs(scans[0], 0)})
    top = max(int(t) >> 8 for t in scans[0]["trailer"])
    assert len(keys) > 100
    rng = random.Random(11)
    tombs = []
    for _ in range(40):
        i = rng.randrange(len(keys) - 8)
        tombs.append((keys[i], keys[i + rng.randrange(1, 8)], top + rng.randrange(0, 3)))
    runs = [dev_run(run_kvs(tombs[r::2], comparer)) for r in range(2)]
    hosts = [r.to_host() for r in runs]
    union = merge_host(scans, comparer=comparer)
    plain = device_result(read(tables, lo, up))
    for snapshot in (MAX, top + 1):
        got = device_result(read(tables, lo, up, snapshot=snapshot, range_dels=runs))
        cov, st = cover_host(hosts, union[0], comparer, snapshot)
        assert st == 0
        want = visible_host(union[0], comparer=comparer, snapshot=snapshot, cover=cov)
        assert_same_batch(got[0], want[0], snapshot)
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), snapshot
        assert 0 < got[0]["n_kv"] < plain[0]["n_kv"] or snapshot != MAX
    # level by level: table 1 shallower than table 0, the runs' levels the other way round
    got = device_result(read(tables, lo, up, range_dels=runs, levels=[1, 0], range_del_levels=[0, 1]))
    cov, st = cover_host(hosts, union[0], comparer, MAX, levels=[0, 1], src_run=union[1], run_levels=[1, 0])
    assert st == 0 and (cov == N.PBL_RANGEDEL_ALL).any()
    want = visible_host(union[0], comparer=comparer, cover=cov)
    assert_same_batch(got[0], want[0], "levels")
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    # no tombstones: the call sequence without range deletions
    none = device_result(read(tables, lo, up, range_dels=[]))
    assert_same_batch(none[0], plain[0], "none")
    assert none[1].tolist() == plain[1].tolist()
    # a run that is not fragmented is reported, not ignored
    from pebble_amd.batch import DecodeError
    bad = dev_run([(b"b", make_trailer(9, RANGEDEL), b"a")])
    with pytest.raises(DecodeError):
        read(tables, lo, up, range_dels=[bad])


def test_golden_tables_hold_no_range_deletions():
    from pebble_amd.sstable import Table
    from tableutil import TABLES, table_bytes
    for name in sorted(TABLES):
        assert Table(table_bytes(name)).range_dels() is None, name
    # the h tables do hold some: 17 fragments at sequence number 0, which delete nothing, one of them empty ([a, a))
    t = Table(table_bytes("h_no_compression.sst"))
    run = t.range_dels()
    h = run.to_host()
    assert h["n_kv"] == 17 and all(int(x) == 15 for x in h["trailer"])
    assert build_set([run], t.comparer()).to_host()["status_mask"] == 0
