"""Columnar keyspan blocks without a GPU: the reference's own
blocks and iterator outputs (tests/golden/keyspan.json) pin the Python decoder
of tests/keyspanutil.py; pebble_amd.keyspan.Writer is byte-exact against the
golden block bytes; pbl_keyspan_decode_host agrees with the Python decoder on
the goldens and on random valid and broken blocks, on every array and total."""
import random

import pytest

from keyspanutil import (BOUNDS, HEADER, assert_same, block_of_spans, break_block, decode_block, expected, gap_blocks,
                         load_golden, random_spans, sized)
from pebble_amd import _native as N
from pebble_amd.batch import Capacity
from pebble_amd.keyspan import Writer, decode_host

G = load_golden()
BLOCKS = {b["name"]: b for b in G["blocks"]}


def golden_spans(spans, synthetic_seq_num=0):
    """[(start, end, trailer, suffix, value)] of a golden span list, one per key."""
    return [(s["start"].encode(), s["end"].encode(), seq << 8 | kind, suffix.encode(), value.encode())
            for s in spans for seq, kind, suffix, value in s["keys"]]


def writer_spans(spans):
    return [(s["start"].encode(), s["end"].encode(), [(seq << 8 | kind, suffix.encode(), value.encode())
                                                      for seq, kind, suffix, value in s["keys"]]) for s in spans]


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_python_decoder_reads_the_reference_blocks(name):
    b = BLOCKS[name]
    blk = bytes.fromhex(b["hex"])
    st, kvs = decode_block(blk)
    assert st == 0 and [kv[:5] for kv in kvs] == golden_spans(b["spans"])
    for w in b["walks"]:
        st, kvs = decode_block(blk, w["synthetic_seq_num"])
        want = golden_spans(w["spans"])
        if w["synthetic_seq_num"]:  # the walk prints the synthetic sequence number
            assert all(t >> 8 == w["synthetic_seq_num"] for _, _, t, _, _ in want)
        assert st == 0 and [kv[:5] for kv in kvs] == want


def test_the_gap_block_is_among_the_goldens():
    b = BLOCKS["keyspan_block/2"]
    st, kvs = decode_block(bytes.fromhex(b["hex"]))
    assert st == 0 and [kv[5] for kv in kvs] == [0, 2] and [kv[6] for kv in kvs] == [0, 1]


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_writer_is_byte_exact(name):
    b = BLOCKS[name]
    assert block_of_spans(writer_spans(b["spans"])).hex() == b["hex"]


def test_writer_of_nothing_is_the_reference_empty_block():
    blk = Writer().finish()
    assert len(blk) == 37 and decode_block(blk) == (0, [])  # keyspan_block's `init`: size=37


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_host_form_on_the_goldens(name):
    b = BLOCKS[name]
    blk = bytes.fromhex(b["hex"])
    for ssn in [0] + [w["synthetic_seq_num"] for w in b["walks"]]:
        assert_same(decode_host([blk], extras=True, synthetic_seq_num=ssn), expected([blk], ssn), (name, ssn))
    assert_same(decode_host([blk]), expected([blk], extras=False), name, extras=False)


def test_host_form_on_all_goldens_as_one_batch():
    blocks = [bytes.fromhex(b["hex"]) for b in G["blocks"]]
    got = decode_host(blocks, extras=True)
    assert_same(got, expected(blocks), "batch")
    assert got["n_kv"] == sum(len(s["keys"]) for b in G["blocks"] for s in b["spans"])


def test_host_form_on_random_blocks():
    rng = random.Random(5)
    for it in range(150):
        blocks = [block_of_spans(random_spans(rng, rng.randrange(1, 40), range_keys=it % 2 == 0))
                  for _ in range(rng.randrange(1, 4))]
        ssn = rng.choice((0, 0, 77))
        assert_same(decode_host(blocks, extras=True, synthetic_seq_num=ssn), expected(blocks, ssn), it)


def test_host_form_on_broken_blocks():
    rng = random.Random(6)
    seen = set()
    for it in range(600):
        good = block_of_spans(random_spans(rng, rng.randrange(1, 12)))
        blocks = [good, break_block(rng, good), good]
        want = expected(blocks)
        assert_same(decode_host(blocks, extras=True), want, it)
        seen.add(int(want["blk_status"][1]))
        assert int(want["blk_status"][0]) == 0 and int(want["blk_status"][2]) == 0
    assert {0, HEADER, BOUNDS} <= seen


@pytest.mark.parametrize("case", gap_blocks(), ids=[c[0] for c in gap_blocks()])
def test_gaps_and_their_corruptions(case):
    name, blk, status = case
    want = expected([blk])
    assert int(want["blk_status"][0]) == status, name
    assert_same(decode_host([blk], extras=True), want, name)
    if name == "gap first":
        assert want["entry_off"].tolist() == [2, 3] and want["span"].tolist() == [1, 1]
    if name == "rows past the last boundary":
        assert want["entry_off"].tolist() == [1]


def test_host_form_overflow_and_size():
    blk = block_of_spans(random_spans(random.Random(8), 20))
    want = expected([blk])
    full = Capacity(want["n_kv"], want["key_bytes_total"], want["val_bytes_total"], 0)
    ecap = (len(want["suffix_bytes"]), len(want["value_bytes"]))
    assert_same(decode_host([blk], extras=True, cap=full, extra_cap=ecap), want, "exact")
    for short in (Capacity(full.kv - 1, full.key, full.val, 0), Capacity(full.kv, full.key - 1, full.val, 0),
                  Capacity(full.kv, full.key, full.val - 1, 0)):
        assert_same(decode_host([blk], extras=True, cap=short, extra_cap=ecap), sized(want), short)
    for ec in ((ecap[0] - 1, ecap[1]), (ecap[0], ecap[1] - 1)):
        assert_same(decode_host([blk], extras=True, cap=full, extra_cap=ec), sized(want), ec)


def test_invalid_arguments():
    import ctypes
    lib = N.lib()
    assert lib.pbl_keyspan_decode_host(None, None, None) == N.PBL_INVALID_ARG
    assert lib.pbl_keyspan_decode(None, 0, None, None, None, 0, None) == N.PBL_INVALID_ARG
    assert lib.pbl_keyspan_workspace_bytes(1, 100) > lib.pbl_keyspan_workspace_bytes(1, 0) > 0
    buf = (ctypes.c_uint64 * 16)()
    n = lib.pbl_keyspan_struct_layout(ctypes.cast(buf, ctypes.c_void_p), 16)
    S = N.KeyspanExtraC
    assert list(buf[:n]) == [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
