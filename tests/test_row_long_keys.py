"""Row keys longer than the 32 KiB LDS key buffer, without a GPU: the
workspace entry that sizes the key spill slots (pbl_workspace_bytes_for, ABI
v9), and the oracle on the blocks the GPU test decodes (every legal shape is
status 0 and holds a key past the buffer, so the GPU comparison is not
vacuous)."""
import numpy as np
import pytest

import oracle
from longkeyutil import C, corrupt_blocks, long_key_blocks, slot_loop_blocks
from pebble_amd import _native as N

G = N.PBL_LONGKEY_WGS


def test_abi_version_is_9():
    assert N.ABI_VERSION == 9
    assert N.lib().pbl_abi_version() == 9


@pytest.mark.parametrize("n", [0, 1, 7, 4096, 100000])
def test_workspace_bytes_for_short_blocks_is_the_old_size(n):
    L = N.lib()
    for ln in (0, 1, 4096, 32767, 32768):
        assert L.pbl_workspace_bytes_for(n, ln) == L.pbl_workspace_bytes(n)


@pytest.mark.parametrize("n", [1, 7, 4096])
def test_workspace_bytes_for_grows_by_the_slots(n):
    L = N.lib()
    base = L.pbl_workspace_bytes(n)
    assert base % 16 == 0  # the slots start 16-B aligned
    for ln in (32769, 32784, 40960, 102401, 200000, (1 << 32) - 1):
        assert L.pbl_workspace_bytes_for(n, ln) == base + G * ((ln + 15) // 16 * 16)


def _max_key_len(blk: bytes) -> int:
    """The longest internal key of a row block, by its entry headers."""
    nres = int.from_bytes(blk[-4:], "little")
    end, off, best = len(blk) - 4 * (1 + nres), 0, 0
    while off < end:
        v = []
        for _ in range(3):
            x, n = oracle.decode_varint(blk[off:off + 5])
            v.append(x)
            off += n
        best = max(best, v[0] + v[1])
        off += v[1] + v[2]
    return best


@pytest.mark.parametrize("ri", [1, 2, 16])
def test_oracle_decodes_every_generated_block(ri):
    named = long_key_blocks(ri)
    assert len(named) >= 15
    for name, blk in named:
        assert len(blk) > C and _max_key_len(blk) >= C, name
        for flags in (0, N.PBL_ROW_RAW_KEYS, N.PBL_ROW_VALUE_PREFIX):
            st, kvs, _ = oracle.rowblk_decode_block(blk, flags)
            assert st == 0 and 2 <= len(kvs) <= 6, (name, flags, st)
    past = [name for name, blk in named if _max_key_len(blk) > C]
    assert len(past) >= len(named) - 2  # (all but the key that just fits)
    for blk in slot_loop_blocks(3):
        assert oracle.rowblk_decode_block(blk, 0)[0] == 0 and 40 * 1024 < len(blk) < 42 * 1024


def test_oracle_hides_the_obsolete_long_keys():
    for name, blk in long_key_blocks(2):
        if not name.startswith("hide"):
            continue
        plain = oracle.rowblk_decode_block(blk, 0)
        hid = oracle.rowblk_decode_block(blk, 0, (0, True, b"", b"", 0))
        assert plain[0] == 0 and hid[0] == 0
        assert len(plain[1]) == 4 and len(hid[1]) == 2
        assert len(hid[1][1][0]) > C  # the visible key after the hidden one is a long one


def test_oracle_rejects_the_corrupt_blocks():
    for ri in (1, 2, 16):
        for name, blk in corrupt_blocks(ri):
            assert oracle.rowblk_decode_block(blk, 0)[0] == N.PBL_CORRUPT_BOUNDS, name
