"""The row-block encoder on the device (pbl_rowenc_size + pbl_rowenc_batch)
against the host form (pbl_rowenc_batch_host), every output array exact; against
the Python model on the small cases; the reference's table byte for byte; the
round trip through the device decode.  Shapes: the smallest at which each piece
can go wrong (tests/rowencutil.py's shared cases), and past one wave, one tile
and one doubling round of every per-stream and per-KV loop."""
import numpy as np
import pytest
import torch

from pebble_amd import _native as N
from pebble_amd.batch import decode
from pebble_amd.rowenc import RowEncOptions, encode, encode_host
from rowencutil import (HAMLET_OPTS, MERGE, SET, assert_round_trip, assert_same, block_bytes, edge_cases, hamlet,
                        host_of, model_encode, opts_of, random_cases, seq_stream, tr, upload)

pytestmark = pytest.mark.gpu


def run(host, opts, ctx, model=False, round_trip=True, **caps):
    dev = encode(upload(host, "cuda:0"), opts, **caps)
    g = dev.to_host()
    assert_same(g, encode_host(host, opts, **caps), ctx)
    if model:
        assert_same(g, model_encode(host, opts), ctx + " (model)")
    if round_trip:
        d = decode(dev.block_batch(), exact=True).to_host() if dev.n_blocks else None
        if d is not None:
            assert_round_trip(host, g, opts, decoded=d, ctx=ctx)
    return g


@pytest.mark.parametrize("case", random_cases() + edge_cases(), ids=lambda c: c[0])
def test_device_against_host_form_and_model(case):
    name, opts, streams = case
    run(host_of(streams), opts, name, model=True)


def test_reference_table_byte_for_byte():
    blocks, host = hamlet()
    g = run(host, HAMLET_OPTS, "hamlet")
    assert g["n_blocks"] == 14
    for b, want in enumerate(blocks):
        assert block_bytes(g, b) == want, b


@pytest.mark.parametrize("n_streams", [70, 1100])
def test_many_streams(n_streams):
    """Past one wave and one tile of every per-stream loop; empty and bad
    streams among them."""
    streams = []
    for q in range(n_streams):
        if q % 13 == 5:
            streams.append(None)
        elif q % 7 == 3:
            streams.append([])
        else:
            streams.append([(b"s%04d-%03d" % (q, i), tr(9 + (i & 1)), b"v" * (i % 9)) for i in range(1 + q % 23)])
    g = run(host_of(streams), opts_of(3, 96, flags=(True, True, False)), f"{n_streams} streams")
    assert g["n_bad_streams"] == sum(1 for s in streams if s is None)


def test_one_long_stream_thousands_of_blocks():
    """About 40 K 12-byte KVs at target 256: every doubling round, and blocks
    straddling every tile edge of the scans."""
    kvs = [(b"%06d" % i, tr(7), b"ab") for i in range(40000)]
    for ri in (16, 3):
        g = run(host_of([kvs]), opts_of(ri, 256), f"long stream ri={ri}", round_trip=ri == 16)
        assert g["n_blocks"] > 2000


def test_blocks_of_many_entries():
    """Blocks of more than 64 and more than 256 entries (a wave's steps, a tile)."""
    kvs = [(b"%05d" % i, tr(7, MERGE if i % 5 == 0 else SET), b"") for i in range(9000)]
    for flags in ((False, False, False), (True, True, False)):
        g = run(host_of([kvs, kvs[:100], kvs[:300]]), opts_of(16, 32768, flags=flags), f"big blocks {flags}")
        assert int(g["block_n_kv"].max()) > 256 and 64 < int(g["block_n_kv"][-2]) <= 256


def test_long_values_and_keys():
    """A value far longer than a wave's step of short copies (the whole-wave
    copy), beside short ones; a long key shared and unshared."""
    big = bytes(range(256)) * 300
    kvs = [(b"a", tr(5), b"x"), (b"b", tr(5), big), (b"c", tr(5), b"y" * 513), (b"d" + b"k" * 5000, tr(5), b"z" * 512),
           (b"d" + b"k" * 5000 + b"e", tr(5), b""), (b"e", tr(5), big[:70001])]
    for flags in ((False, False, False), (True, False, False)):
        run(host_of([kvs]), opts_of(2, 4096, flags=flags), f"long values {flags}", model=True)


def test_overflow_reports_every_size():
    host = host_of([[(b"%04d" % i, tr(3), b"v" * 20) for i in range(400)], [(b"a", tr(1), b"")]])
    opts = RowEncOptions(4, 128, 90)
    full = run(host, opts, "fits")
    for caps in ({"block_cap": 2}, {"blocks_cap": 64}):
        g = encode(upload(host, "cuda:0"), opts, **caps).to_host()
        assert g["status_mask"] == 1 << N.PBL_OVERFLOW, caps
        for k in ("n_blocks", "block_bytes", "n_restarts"):
            assert g[k] == full[k], (caps, k)
        assert np.array_equal(g["stream_block_base"], full["stream_block_base"])
        assert np.array_equal(g["stream_status"], full["stream_status"])


def test_unsized_batch_matches_sized():
    """pbl_rowenc_batch without PBL_ROWENC_SIZED computes the partition itself."""
    import ctypes
    host = host_of([seq_stream(500, vlen=7), seq_stream(3)])
    opts = opts_of(5, 200)
    want = encode_host(host, opts)
    b = upload(host, "cuda:0")
    L = N.lib()
    n_kv, nb = host["n_kv"], 2
    ws = torch.empty(int(L.pbl_rowenc_workspace_bytes(nb, n_kv)), dtype=torch.uint8, device="cuda:0")
    u = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device="cuda:0")  # noqa: E731
    blocks, off, first = u(want["block_bytes"], torch.uint8), u(want["n_blocks"], torch.int64), u(want["n_blocks"], torch.int64)
    ln, bst, nkv = (u(want["n_blocks"], torch.int32) for _ in range(3))
    sbb, sst, tot = u(nb + 1, torch.int64), u(nb, torch.int32), u(ctypes.sizeof(N.RowEncTotalsC), torch.uint8)
    cin, co = N.RowEncInC(b.c_struct(), nb, 0, n_kv), opts.c_struct()
    oo = N.RowEncOutC(blocks.data_ptr(), off.data_ptr(), ln.data_ptr(), bst.data_ptr(), first.data_ptr(), nkv.data_ptr(),
                      sbb.data_ptr(), sst.data_ptr(), None, tot.data_ptr(), want["block_bytes"], want["n_blocks"])
    st = torch.cuda.current_stream()
    rc = L.pbl_rowenc_batch(ctypes.byref(cin), ctypes.byref(co), ctypes.byref(oo), ctypes.c_void_p(ws.data_ptr()),
                            ws.numel(), 0, ctypes.c_void_p(st.cuda_stream))
    assert rc == N.PBL_OK
    st.synchronize()
    t = N.RowEncTotalsC.from_buffer_copy(tot.cpu().numpy().tobytes())
    assert (t.n_blocks, t.block_bytes, t.n_restarts, t.status_mask) == (want["n_blocks"], want["block_bytes"],
                                                                       want["n_restarts"], 0)
    assert np.array_equal(blocks.cpu().numpy(), want["blocks"])
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want["block_off"])
    assert np.array_equal(ln.cpu().numpy().view(np.uint32), want["block_len"])


def test_compact_tables_to_blocks():
    """decode -> scan -> merge -> compact -> encode: every range's kept KVs come
    back from the blocks, and the blocks are the host form's over the result."""
    from pebble_amd.batch import BlockBatch
    from pebble_amd.compact import compact_tables_to_blocks
    from pebble_amd.rowblk import Writer
    from pebble_amd.scan import scan

    class BlocksTable:
        def __init__(self, kvs, per_block):
            blocks = []
            for i in range(0, len(kvs), per_block):
                w = Writer(4)
                for k, t, v in kvs[i:i + per_block]:
                    w.add(k, t, v)
                blocks.append(w.finish())
            self.d = decode(BlockBatch.from_blocks(blocks, "cuda", N.PBL_FMT_ROW, 0))

        def comparer(self):
            return N.PBL_CMP_DEFAULT

        def scan(self, lowers, uppers, hide_obsolete_points=False):
            return scan(self.d, lowers, uppers, comparer=N.PBL_CMP_DEFAULT, hide_obsolete_points=hide_obsolete_points)

    kvs = [(b"key%03d" % (i // 3), tr(900 - i, (SET, MERGE, SET)[i % 3]), b"v%d" % i) for i in range(600)]
    tables = [BlocksTable(kvs[r::2], 50 + 20 * r) for r in range(2)]
    opts = opts_of(4, 300, flags=(True, True, False))
    res, enc = compact_tables_to_blocks(tables, [None, b"key100"], [b"key100", None], opts, snapshots=(500,))
    kept = res.batch.to_host()
    g = enc.to_host()
    assert g["n_blocks"] > 4 and g["stream_block_base"][1] > 0 and not g["status_mask"]
    assert_same(g, encode_host(kept, opts), "compact_tables_to_blocks")
    assert_round_trip(kept, g, opts, decoded=decode(enc.block_batch(), exact=True).to_host())
    with pytest.raises(ValueError, match="comparer"):
        compact_tables_to_blocks(tables, [None], [None], opts_of(4, 300, N.PBL_CMP_CRDB))
