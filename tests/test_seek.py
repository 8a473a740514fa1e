"""Batched seeks without a GPU: the ABI additions (pbl_seek_struct_layout, the
workspace size, every invalid-argument return, all before any device call) and
pbl_seek_batch_host -- the same seek_one the device kernel instantiates --
against the one-key host iterator (DataIter) over the oracle's decoded arrays:
both ops, both modes, HideObsoletePoints on and off, the three comparers."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import Writer, make_trailer
from pebble_amd.seek import pack_keys, seek_host
from seekutil import Seq, assert_seek, block_of, expected, keyfn, sorted_keys


def decoded(blocks, flags=0):
    off, lens, pos = [], [], 0
    for b in blocks:
        off.append(pos)
        lens.append(len(b))
        pos += (len(b) + 15) // 16 * 16
    buf = np.zeros(pos + 16, np.uint8)
    for o, b in zip(off, blocks):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return oracle.rowblk_decode_batch(buf, np.array(off, np.uint64), np.array(lens, np.uint32), flags)


def test_struct_layout_matches_the_ctypes_mirrors():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    n = L.pbl_seek_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 64)
    exp = []
    for S in (N.SeekQueriesC, N.SeekOutC):
        exp.append(ctypes.sizeof(S))
        exp += [getattr(S, f).offset for f, _ in S._fields_]
    assert list(buf[:n]) == exp
    assert L.pbl_abi_version() == 9


def test_workspace_bytes():
    L = N.lib()
    prev = 0
    for nb in (0, 1, 2, 63, 1023, 1024, 1025, 4096, 65536, 1 << 20, (1 << 32) - 1):
        w = int(L.pbl_seek_workspace_bytes(nb))
        assert w > 0 and w % 16 == 0 and w >= prev, (nb, w)
        assert w >= 32 * nb  # one 32-B fence record per block
        prev = w


class _Args:
    """A syntactically valid argument set over host memory posing as device
    memory: every call below must return before it touches any of it."""

    def __init__(self):
        self.arr = np.zeros(64, np.uint64)
        p = self.arr.ctypes.data
        self.d = N.DecodeOutC()
        for f in ("kv_flags", "key_off", "key_bytes", "blk_kv_base", "blk_key_base", "blk_status"):
            setattr(self.d, f, p)
        self.q = N.SeekQueriesC(p, p, p, 4, N.PBL_CMP_DEFAULT, N.PBL_SEEK_GE, 0)
        self.out = N.SeekOutC(p, p, p)
        self.ws = np.zeros(4096 + 16, np.uint8)
        a = self.ws.ctypes.data
        self.ws_ptr = (a + 15) // 16 * 16
        self.ws_bytes = 4096

    def batch(self, ws="own", ws_bytes=None):
        ptr = self.ws_ptr if ws == "own" else ws
        return N.lib().pbl_seek_batch(ctypes.byref(self.d), 4, ctypes.byref(self.q), ctypes.byref(self.out),
                                      ctypes.c_void_p(ptr) if ptr else None,
                                      self.ws_bytes if ws_bytes is None else ws_bytes, None)


def test_invalid_arguments_return_before_any_device_call():
    L = N.lib()
    a = _Args()
    a.q.comparer = 3
    assert a.batch() == N.PBL_INVALID_ARG
    a = _Args()
    a.q.op = 2
    assert a.batch() == N.PBL_INVALID_ARG
    a = _Args()
    a.out.kv = None
    assert a.batch() == N.PBL_INVALID_ARG
    a = _Args()
    a.q.key_off = None
    assert a.batch() == N.PBL_INVALID_ARG
    a = _Args()
    assert a.batch(ws=a.ws_ptr + 8) == N.PBL_INVALID_ARG           # misaligned workspace
    assert a.batch(ws_bytes=int(L.pbl_seek_workspace_bytes(4)) - 1) == N.PBL_INVALID_ARG  # short workspace
    a.q.block = None
    assert a.batch(ws=None, ws_bytes=0) == N.PBL_INVALID_ARG      # table mode without a workspace
    a = _Args()
    a.q.hide_obsolete_points = 1
    a.d.kv_flags = None
    assert a.batch() == N.PBL_INVALID_ARG
    a = _Args()
    a.d.blk_status = None
    assert a.batch() == N.PBL_INVALID_ARG
    # n == 0: PBL_OK without a launch (per-block mode needs no workspace)
    a = _Args()
    a.q.n = 0
    assert a.batch(ws=None, ws_bytes=0) == N.PBL_OK
    # pbl_seek_prepare
    prep = lambda d, cmp, ws, nbytes: L.pbl_seek_prepare(ctypes.byref(d), 4, cmp,  # noqa: E731
                                                         ctypes.c_void_p(ws) if ws else None, nbytes, None)
    a = _Args()
    assert prep(a.d, 3, a.ws_ptr, a.ws_bytes) == N.PBL_INVALID_ARG
    assert prep(a.d, 0, None, 0) == N.PBL_INVALID_ARG
    assert prep(a.d, 0, a.ws_ptr + 8, a.ws_bytes) == N.PBL_INVALID_ARG
    assert prep(a.d, 0, a.ws_ptr, int(L.pbl_seek_workspace_bytes(4)) - 1) == N.PBL_INVALID_ARG
    a.d.key_off = None
    assert prep(a.d, 0, a.ws_ptr, a.ws_bytes) == N.PBL_INVALID_ARG
    # the host entry point shares the checks
    a = _Args()
    a.q.op = 2
    assert L.pbl_seek_batch_host(ctypes.byref(a.d), 4, ctypes.byref(a.q), ctypes.byref(a.out)) == N.PBL_INVALID_ARG


def _ordered_batch(rng, comparer, n_blocks, seq):
    """Blocks whose user keys ascend over the whole batch (a table's data
    blocks), an empty block and a corrupt one among them."""
    kf = keyfn(rng, comparer, roaches=(b"k1", b"k2", b"k3", b"k4", b"k5"))
    keys = sorted_keys(comparer, [kf() for _ in range(40 * n_blocks)])
    cuts = sorted(rng.sample(range(1, len(keys)), n_blocks - 1))
    parts = [keys[a:b] for a, b in zip([0] + cuts, cuts + [len(keys)])]
    blocks = [block_of(rng, seq, p) for p in parts]
    blocks.insert(2, Writer(16).finish())       # decodes, holds nothing
    blocks.insert(4, b"\x00\x00\x00\x00")       # zero restarts: PBL_CORRUPT_NO_RESTARTS
    return blocks, keys, kf


@pytest.mark.parametrize("comparer", [N.PBL_CMP_DEFAULT, N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB])
def test_host_seek_matches_data_iter(comparer):
    rng = random.Random(comparer + 17)
    blocks, keys, kf = _ordered_batch(rng, comparer, 6, Seq())
    d = decoded(blocks)
    assert int(d["blk_status"][4]) != 0 and int(d["blk_status"][2]) == 0
    nb = len(blocks)
    probes = keys + [kf() for _ in range(60)] + [b""]
    if comparer == N.PBL_CMP_DEFAULT:
        probes += [k + b"\x00" for k in keys[::3]] + [k[:-1] for k in keys[::3]] + [b"\xff" * 40]
    for hide in (False, True):
        for op in ("ge", "lt"):
            # table mode
            got = seek_host(d, probes, op=op, comparer=comparer, hide_obsolete_points=hide)
            assert_seek(got, expected(d, probes, op, comparer, None, hide), (comparer, op, hide, "table"))
            # per-block mode: every probe against a random block, past-the-end ids too
            blk = [rng.randrange(nb + 2) for _ in probes]
            got = seek_host(d, probes, op=op, comparer=comparer, blocks=blk, hide_obsolete_points=hide)
            assert_seek(got, expected(d, probes, op, comparer, blk, hide), (comparer, op, hide, "block"))


def test_host_seek_per_block_ignores_batch_order():
    """Per-block mode makes no assumption about the order of blocks."""
    rng = random.Random(5)
    seq = Seq()
    kf = keyfn(rng, N.PBL_CMP_DEFAULT)
    blocks = [block_of(rng, seq, sorted_keys(N.PBL_CMP_DEFAULT, [kf() for _ in range(rng.randrange(1, 60))]))
              for _ in range(6)]
    d = decoded(blocks)
    probes = [kf() for _ in range(200)]
    blk = [rng.randrange(6) for _ in probes]
    for hide in (False, True):
        for op in ("ge", "lt"):
            got = seek_host(d, probes, op=op, comparer=N.PBL_CMP_DEFAULT, blocks=blk, hide_obsolete_points=hide)
            assert_seek(got, expected(d, probes, op, N.PBL_CMP_DEFAULT, blk, hide), (op, hide))


def test_host_seek_hidden_runs_cross_blocks():
    """Block 0's last two KVs, all of block 1 and block 2's first KV obsolete:
    SeekGE of block 0's last key lands in block 2 and SeekLT of block 2's
    second key in block 0; per-block mode gives NONE for both."""
    seq = Seq()

    def blk(keys, obs):
        w = Writer(2)
        for k, o in zip(keys, obs):
            w.add_with_optional_value_prefix(k, seq.next(), o, b"v", len(k), False, 0, False)
        return w.finish()

    b0 = [b"a1", b"a2", b"a3", b"a4"]
    b1 = [b"b1", b"b2", b"b3"]
    b2 = [b"c1", b"c2", b"c3"]
    d = decoded([blk(b0, [0, 0, 1, 1]), blk(b1, [1, 1, 1]), blk(b2, [1, 0, 0])])
    C = N.PBL_CMP_DEFAULT
    kv, b, f = seek_host(d, [b"a4"], op="ge", comparer=C, hide_obsolete_points=True)
    assert (int(kv[0]), int(b[0]), int(f[0])) == (8, 2, 0)  # c2
    kv, b, f = seek_host(d, [b"c2"], op="lt", comparer=C, hide_obsolete_points=True)
    assert (int(kv[0]), int(b[0])) == (1, 0)  # a2
    kv, b, f = seek_host(d, [b"a4", b"c2"], op="ge", comparer=C, blocks=[0, 1], hide_obsolete_points=True)
    assert kv.tolist() == [N.PBL_SEEK_NONE, N.PBL_SEEK_NONE] and f.tolist() == [0, 0]
    kv, b, f = seek_host(d, [b"c2"], op="lt", comparer=C, blocks=[2], hide_obsolete_points=True)
    assert kv.tolist() == [N.PBL_SEEK_NONE]
    probes = b0 + b1 + b2 + [b"", b"a", b"b", b"c", b"d"]
    for hide in (False, True):
        for op in ("ge", "lt"):
            got = seek_host(d, probes, op=op, comparer=C, hide_obsolete_points=hide)
            assert_seek(got, expected(d, probes, op, C, None, hide), (op, hide))


def test_host_seek_flags():
    w = Writer(16)
    for i, k in enumerate([b"a@10", b"a@3", b"b@5"]):
        w.add(k, make_trailer(9 - i, 1), b"")
    d = decoded([w.finish()])
    T = N.PBL_CMP_TESTKEYS
    kv, b, f = seek_host(d, [b"a@10", b"a@7", b"a@5_synthetic", b"a", b"b@9", b"c"], op="ge", comparer=T)
    assert kv.tolist() == [0, 1, 1, 0, 2, N.PBL_SEEK_NONE]
    E, P = N.PBL_SEEK_EXACT, N.PBL_SEEK_SAME_PREFIX
    assert f.tolist() == [E | P, P, P, P, P, 0]
    kv, b, f = seek_host(d, [b"a@10", b"b@5", b"b"], op="lt", comparer=T)
    assert kv.tolist() == [N.PBL_SEEK_NONE, 1, 1] and f.tolist() == [0, 0, 0]


def test_pack_keys_pads_sixteen_bytes():
    buf, off = pack_keys([b"ab", b"", b"cde"])
    assert off.tolist() == [0, 2, 2, 5] and buf.size == 5 + 16 and bytes(buf[:5]) == b"abcde"
