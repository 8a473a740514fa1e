"""Every colblk column encoding on every device route: the directed matrix of
tests/colencutil.py (every Uint width and delta bit per column, both sides of
the 6144 / 8192 / 12288-byte stage thresholds, the bitmap word boundaries and
the 512-byte tail, duplicate runs across bundle boundaries) and its negative
blocks as one batch per schema, at block alignments 16, 8 and 1 (1: the wave
form drops its stage and every width goes through g_le's unaligned loop),
through the two-pass wave form with the fixed and the PBL_BATCH_VARLEN stage,
the pipeline and the one-block-per-workgroup kernel; then the fused hide, mixed
row + colblk batches, the tiering columns, the exact and the overflow-retry
decodes.  Each decode is compared bit-exactly with the oracle's, and every
PBL_OK block with what its writer was given (tests/test_colblk_encodings.py
pins the cells and the oracle's side)."""
import functools

import numpy as np
import pytest

import oracle
from colencutil import matrix, negatives, tiering_matrix
from pebble_amd import _native as N
from pebble_amd.batch import BlockBatch, Capacity, decode
from pebble_amd.colblk import SCHEMA_CRDB1, SCHEMA_DEFAULT
from pebble_amd.rowblk import gen_row_blocks, kvs_of_block
from test_rowblk_gpu import assert_same, pack

pytestmark = pytest.mark.gpu
KERNELS = {"wave": 0, "wave_varlen": N.PBL_BATCH_VARLEN, "pipe": N.PBL_KERNEL_PIPE, "single": N.PBL_KERNEL_SINGLE}
SCHEMAS = [SCHEMA_DEFAULT, SCHEMA_CRDB1]
ALIGNS = (16, 8, 1)
HIDE, TIER = N.PBL_ROW_HIDE_OBSOLETE, N.PBL_COL_TIERING
META = ("tiering_span_id", "tiering_attr")


@functools.lru_cache(maxsize=None)
def entries(schema):
    """The schema's batch: (context, block, writer-input expectation) per block,
    the matrix first, then the negative blocks (each with its source's
    expectation, which holds where the oracle decodes it)."""
    out = [(c.ctx, c.block, [e[:4] for e in c.exp]) for c in matrix() if c.schema == schema]
    out += [(f"{name}: {src.ctx}", blk, [e[:4] for e in src.exp]) for name, s, blk, src in negatives() if s == schema]
    return out


@functools.lru_cache(maxsize=None)
def packed(schema, align):
    """(buf, off, lens, the oracle's decode), computed once per alignment."""
    buf, off, lens = pack([blk for _, blk, _ in entries(schema)], align)
    return buf, off, lens, oracle.decode_batch(buf, off, lens, schema)


def first_difference(g, o, ents):
    """The first block whose status or KVs differ from the oracle's."""
    for b, (ctx, _, _) in enumerate(ents):
        if ctx is None:
            continue
        try:
            same = g["blk_status"][b] == o["blk_status"][b] and kvs_of_block(g, b) == kvs_of_block(o, b)
        except Exception:  # (bases that make no sense)
            same = False
        if not same:
            return f"block {b} [{ctx}] status {g['blk_status'][b]} (oracle {o['blk_status'][b]})"
    return "none by block (totals or bases)"


def same_as(g, o, ents, ctx, expect=lambda exp: exp, meta=None):
    """g is the oracle's o bit for bit, and every PBL_OK block holds what its
    writer was given (`expect` applies the batch's transforms to that)."""
    try:
        assert_same(g, o, ctx)
        for k in META if meta is not None else ():
            assert np.array_equal(g[k], o[k]), f"{ctx} array {k} differs"
    except AssertionError as e:
        raise AssertionError(f"{e}; first difference: {first_difference(g, o, ents)}") from None
    n_ok = 0
    for b, (bctx, _, exp) in enumerate(ents):
        if bctx is None or o["blk_status"][b] != N.PBL_OK:
            continue
        n_ok += 1
        got = [(kv.user_key, kv.trailer, kv.value, kv.flags) for kv in kvs_of_block(g, b)]
        assert got == expect(exp), f"{ctx} [{bctx}]"
        if meta is not None:
            kv0, kv1 = int(g["blk_kv_base"][b]), int(g["blk_kv_base"][b + 1])
            got = list(zip(g[META[0]][kv0:kv1].tolist(), g[META[1]][kv0:kv1].tolist()))
            assert got == meta[b], f"{ctx} KVMeta [{bctx}]"
    return n_ok


def run(buf, off, lens, schema, flags, seq=0, block_format=None, **decode_kw):
    bb = BlockBatch.from_host(buf, off, lens, "cuda", schema, flags, block_format=block_format)
    bb.synthetic_seq_num = seq
    return decode(bb, **decode_kw).to_host()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("schema", SCHEMAS)
def test_matrix_on_every_route(schema, kernel):
    ents = entries(schema)
    for align in ALIGNS:
        buf, off, lens, o = packed(schema, align)
        g = run(buf, off, lens, schema, KERNELS[kernel])
        n_ok = same_as(g, o, ents, f"schema={schema} align={align} flags={KERNELS[kernel]:#x} ({kernel})")
        assert n_ok >= sum(c.schema == schema for c in matrix()) and g["n_bad_blocks"] > 0


@pytest.mark.parametrize("seq", [0, 4242])
@pytest.mark.parametrize("schema", SCHEMAS)
def test_matrix_hide_obsolete(schema, seq):
    """PBL_ROW_HIDE_OBSOLETE (fused into the pipeline) with and without a
    synthetic sequence number, against oracle.transform_batch over the plain
    oracle decode."""
    ents = entries(schema)

    def expect(exp):
        return [(k, (seq << 8 | t & 0xFF) if seq else t, v, f) for k, t, v, f in exp if not f & N.PBL_KV_OBSOLETE]

    for align in (8, 1):
        buf, off, lens, plain = packed(schema, align)
        o = oracle.transform_batch(plain, seq, True)
        g = run(buf, off, lens, schema, HIDE, seq)
        same_as(g, o, ents, f"hide schema={schema} align={align} flags={HIDE:#x} seq={seq}", expect)
        assert 0 < g["n_kv"] < plain["n_kv"]


def test_matrix_in_a_mixed_batch():
    """block_format[]: a small row block in front of each colblk block of both
    schemas (the kList size and emit passes, which resolve through the look-back)."""
    rb, ro, rl, _ = gen_row_blocks(17, 8, 1024, 16, 16, 40)
    row = [rb[int(ro[i]):int(ro[i]) + int(rl[i])].tobytes() for i in range(8)]
    ents, fmts = [], []
    for schema in SCHEMAS:
        for i, e in enumerate(entries(schema)):
            ents += [(None, row[i % 8], None), e]
            fmts += [N.PBL_FMT_ROW, schema]
    bf = np.array(fmts, np.uint8)
    for align in (8, 16):
        buf, off, lens = pack([blk for _, blk, _ in ents], align)
        o = oracle.decode_batch(buf, off, lens, 0, bf, 0)
        g = run(buf, off, lens, N.PBL_FMT_ROW, 0, block_format=bf)
        n_ok = same_as(g, o, ents, f"mixed align={align} flags=0x0")
        assert n_ok >= len(matrix())


@functools.lru_cache(maxsize=None)
def tiering_entries(schema):
    cells = [c for c in tiering_matrix() if c.schema == schema]
    return [(c.ctx, c.block, [e[:4] for e in c.exp]) for c in cells], [c.metas for c in cells]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("schema", SCHEMAS)
def test_tiering_columns_on_every_route(schema, kernel):
    """PBL_COL_TIERING over Pebblev8 forms of the threshold blocks and the
    4200-row block: span and attribute widths 0, 1, 2, 4 and 8, read past the
    stages (u_at_any), the KVMeta arrays against the oracle's and the writer's."""
    ents, metas = tiering_entries(schema)
    flags = TIER | KERNELS[kernel]
    for align in ALIGNS:
        buf, off, lens = pack([blk for _, blk, _ in ents], align)
        o = oracle.decode_batch(buf, off, lens, schema, None, flags, meta=True)
        g = run(buf, off, lens, schema, flags, meta=True)
        n_ok = same_as(g, o, ents, f"tiering schema={schema} align={align} flags={flags:#x} ({kernel})", meta=metas)
        assert n_ok == len(ents)


@pytest.mark.parametrize("schema", SCHEMAS)
def test_matrix_exact_and_overflow_retry(schema):
    """The size pass first (exact=True), and a Capacity far too small (the
    overflow-retry path), on the default route."""
    ents = entries(schema)
    buf, off, lens, o = packed(schema, 8)
    same_as(run(buf, off, lens, schema, 0, exact=True), o, ents, f"exact schema={schema} align=8 flags=0x0")
    g = run(buf, off, lens, schema, 0, cap=Capacity(kv=10, key=10, val=10, rst=10))
    same_as(g, o, ents, f"overflow retry schema={schema} align=8 flags=0x0")
