"""Every zstd format feature the device decoder claims (zstd.hip's header
comment), on the CPU: the frames tests/zstdutil.py assembles are held to
facebook/zstd (what it decodes them to, and that it rejects the corrupt
ones), the oracle and the host emulation of zstd_dec.hip.h must agree with it,
and the corpus the GPU tests decode (tests/test_zstd_forms_gpu.py) is held to
a coverage floor by census -- so a bundled libzstd that stops emitting a form
fails here instead of thinning the GPU test out silently.

The emulator compiles zstd_dec.hip.h only (zstd_kernel's code, LDS and global
routes); the batch path (zstd_fast.hip.h) runs only in the GPU tests."""
import os
import random
import shutil
import subprocess

import pytest

import oracle
import zstdutil as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def valid_cases():
    return Z.assembled_forms() + Z.long_count_frames()


def test_assembled_frames_decode_under_libzstd_and_the_oracle():
    for c in valid_cases():
        assert Z.libzstd(c.frame, len(c.want)) == c.want, c.name
        assert oracle.zstd_decompress(c.frame, len(c.want)) == c.want, c.name
        cen = Z.census(c.frame)
        assert all(cen[k] for k in c.feature), (c.name, c.feature, cen)


def test_census_reads_what_the_assembler_wrote():
    """One frame with every header option set, walked back field by field."""
    rng = random.Random(1)
    lits = bytes(rng.choice(b"aaabbc") for _ in range(300))
    blocks = [("raw", b"0123456789" * 3), ("rle", 0x55, 40),
              ("comp", lits, [(1, 4, 3), (1, 5, -1)] * 130, {"ltype": "huffman", "sf": 2, "modes": ("rle", "fse", "predefined"),
                                                            "nseq_bytes": 2}),
              ("comp", lits[:50], [], {"ltype": "treeless", "sf": 0})]
    f, want = Z.frame(blocks, single=False, fcs_bytes=8, checksum=True, did_bytes=2)
    assert Z.libzstd(f, len(want)) == want
    assert Z.census(f) == {"frame": 1, "window_descriptor": 1, "fcs_bytes_8": 1, "dict_id_bytes_2": 1, "checksum": 1,
                           "frame_multi_block": 1, "block_raw": 1, "block_rle": 1, "block_compressed": 2, "lit_huffman": 1,
                           "lit_huffman_sf2": 1, "lit_treeless": 1, "lit_treeless_sf0": 1, "huf_streams_4": 1, "huf_streams_1": 1,
                           "huf_weights_direct": 1, "nseq_2byte": 1, "nseq_0": 1, "ll_rle": 1, "of_fse": 1, "ml_predefined": 1}
    assert Z.first_block_nseq(f + Z.skippable(3) + Z.assembled_forms()[0].frame) == [0, 12]
    fr = Z.walk(f)[0]
    b = fr["blocks"][2]
    assert (b["nseq"], b["regen"], fr["end"]) == (260, 300, len(f))
    assert b["huf_desc"][1] == b["huf_streams"][0] < b["huf_streams"][1] < b["tables"][0] < b["seq_bits"][0] < b["seq_bits"][1]


def test_frames_libzstd_rejects_are_rejected_by_the_oracle():
    cases = Z.rejected_forms()
    assert {"bad_checksum", "rep0_minus_1_is_0", "empty_fourth_stream"} <= {c.name for c in cases}
    for c in cases:
        with pytest.raises(Exception):
            Z.libzstd(c.frame, c.want)
        assert oracle.zstd_decompress(c.frame, c.want) == (-2 if c.feature == "unsupported" else -1), c.name


def test_library_frames_with_a_content_checksum():
    rng = random.Random(3)
    for n in (1, 31, 32, 1000, 40_000, 140_000):
        data = Z.letters(rng, n)
        f = Z.compress(data, 3, checksum=True)
        assert Z.census(f)["checksum"] == 1
        assert Z.libzstd(f, n) == data and oracle.zstd_decompress(f, n) == data
        bad = bytearray(f)
        bad[-1 - rng.randrange(4)] ^= 1 << rng.randrange(8)
        with pytest.raises(Exception):
            Z.libzstd(bytes(bad), n)
        assert oracle.zstd_decompress(bytes(bad), n) == -1


def test_gpu_corpus_coverage_floor():
    """A condition, not a measurement: the GPU tests' corpus holds every
    feature at least twice."""
    cen = Z.corpus_census(Z.zstd_gpu_corpus())
    assert [(k, cen[k]) for k in Z.COVERAGE_FLOOR if cen[k] < 2] == [], sorted(cen.items())
    for c in Z.multi_block_frames():
        one = Z.census(c.frame)
        assert one["frame_multi_block"] and one["lit_treeless"] and one["of_repeat"] and one["ml_repeat"], (c.name, one)
    # the library alone reaches Huffman size formats 0-2; format 3 under 36 KiB comes from the assembler
    lib = Z.corpus_census(Z.library_frames())
    assert all(lib["lit_huffman_sf%d" % i] >= 2 for i in range(3)) and lib["huf_weights_fse"] >= 2, sorted(lib.items())


def test_sequence_area_exhaustion_batch_is_past_the_area():
    batch = Z.exhaustion_batch()
    nseq = [Z.first_block_nseq(f)[0] for f, _ in batch]
    assert all(Z.route(Z.as_is(f, len(d))) == "batch" for f, d in batch)
    assert sum(nseq) > 64 * Z.SEQ_PER_BLOCK, sum(nseq)
    assert Z.min_fallbacks(nseq, 64) >= 3


def test_mixed_exhaustion_batch_is_past_the_area_sized_over_all_its_blocks():
    """The area holds kSeqPerBlock for every block of the batch, whatever its
    codec: the zstd blocks' sequences must exceed that, not their own share."""
    batch = Z.exhaustion_batch_mixed()
    nseq = Z.batch_nseq(batch)
    assert len(batch) == 110 and sorted(ind for _, ind, _ in batch) == [0] * 11 + [1] * 11 + [7] * 88
    assert all(Z.route(bk) == "batch" for bk, ind, _ in batch if ind == 7)
    assert sum(nseq) > len(batch) * Z.SEQ_PER_BLOCK, (sum(nseq), len(batch))
    assert Z.min_fallbacks(nseq, len(batch)) >= 4
    for f, d in Z.dense_blocks():
        assert Z.libzstd(f, len(d)) == d and oracle.zstd_decompress(f, len(d)) == d
    # no run of zstd blocks is free of the other codecs: one follows every fourth
    inds = [ind for _, ind, _ in batch]
    assert all(7 != inds[i + 4] for i in range(0, len(inds) - 4, 5))


def test_min_fallbacks():
    assert Z.min_fallbacks([4096] * 8, 8) == 0
    assert Z.min_fallbacks([4097] * 8, 8) == 1
    assert Z.min_fallbacks([9000, 100, 100, 9000], 4) == 1
    assert Z.min_fallbacks([5000] * 4, 16) == 0


def test_route_wrappers_force_the_routes_they_name():
    """Every frame the GPU tests send down all three routes meets each
    wrapper's forcing condition, bar library frames too large for the LDS
    route, which there may be two of; and each route sees every feature it
    can hold at least twice."""
    cases = Z.library_frames() + Z.assembled_forms()
    on = {"batch": [], "lds": [], "global": []}
    for c in cases:
        n = len(c.want)
        assert n <= Z.K_OUT, c.name
        r = Z.route(Z.as_is(c.frame, n))
        assert r in ("batch", "lds"), (c.name, r)
        one = Z.census(c.frame)
        eligible = not (one["frame_multi_block"] or one["lit_treeless"] or one["dict_id_bytes_0"] == 0
                        or any(one[t + "_repeat"] for t in Z.TABLES) or one["block_compressed"] == 0)
        assert (r == "batch") == eligible, (c.name, r, one)
        on[r].append(c)
        fits = 13 + len(c.frame) <= Z.K_IN
        assert Z.route(Z.skippable_prefix(c.frame, n)) == ("lds" if fits else "global"), c.name
        assert fits or c in Z.library_frames(), c.name
        on["lds" if fits else "global"].append(c)
        assert Z.route(Z.skippable_pad(c.frame, n)) == "global", c.name
        on["global"].append(c)
    prefixed_in_lds = len(on["lds"]) - sum(Z.route(Z.as_is(c.frame, len(c.want))) == "lds" for c in cases)
    assert prefixed_in_lds >= len(cases) - 2 and len(on["batch"]) >= 150, {k: len(v) for k, v in on.items()}
    assert all(Z.route(Z.as_is(c.frame, len(c.want))) == "global" for c in Z.long_count_frames() + Z.multi_block_frames())
    never_batch = {"lit_treeless", "frame_multi_block", "dict_id_bytes_1", "dict_id_bytes_2", "dict_id_bytes_4"} | \
        {t + "_repeat" for t in Z.TABLES}
    for r, held in on.items():
        cen = Z.corpus_census(held)
        floor = [k for k in Z.COVERAGE_FLOOR if k != "nseq_3byte" and not (r == "batch" and k in never_batch)]
        assert [(k, cen[k]) for k in floor if cen[k] < 2] == [], (r, sorted(cen.items()))


# ---- the host emulation of zstd_dec.hip.h -----------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("zemu") / "zstd_emu")
    subprocess.run(["g++", "-O1", "-std=c++20", "-pthread", os.path.join(ROOT, "scripts", "zstd_emu.cpp"), "-o", exe],
                   check=True)
    return exe


def run(emu, tmp_path, raw):
    """The emulated decoder's bytes, or minus its status (-1 corrupt, -2 unsupported: the oracle's codes)."""
    i, o = tmp_path / "in.bin", tmp_path / "out.bin"
    i.write_bytes(raw)
    r = subprocess.run([emu, str(i), str(o)], capture_output=True, text=True, timeout=300)
    return o.read_bytes() if r.returncode == 0 else -r.returncode


def test_emulator_assembled_forms(emu, tmp_path):
    """The LDS route for every form; every third also behind the pad that
    sends it down the global-memory route."""
    for i, c in enumerate(Z.assembled_forms()):
        n = len(c.want)
        routes = (Z.as_is, Z.skippable_pad) if i % 3 == 0 else (Z.as_is,)
        for wrap in routes:
            raw = wrap(c.frame, n)
            want = oracle.zstd_block(raw)
            assert want == c.want
            assert run(emu, tmp_path, raw) == want, (c.name, wrap.__name__)


def test_emulator_rejected_forms(emu, tmp_path):
    for c in Z.rejected_forms():
        for wrap in (Z.as_is, Z.skippable_pad):
            raw = wrap(c.frame, c.want)
            want = oracle.zstd_block(raw)
            assert want == (-2 if c.feature == "unsupported" else -1), c.name
            assert run(emu, tmp_path, raw) == want, (c.name, wrap.__name__)


def test_emulator_long_sequence_count(emu, tmp_path):
    for c in Z.long_count_frames():
        assert Z.census(c.frame)["nseq_3byte"] == 1
        assert run(emu, tmp_path, Z.as_is(c.frame, len(c.want))) == c.want, c.name


def test_emulator_library_huffman_frames(emu, tmp_path):
    """The low-entropy library frames (40 .. 36,864 bytes; the LDS route)."""
    for c in Z.library_frames():
        raw = Z.as_is(c.frame, len(c.want))
        assert oracle.zstd_block(raw) == c.want, c.name
        assert run(emu, tmp_path, raw) == c.want, c.name


def test_emulator_multi_block_treeless_and_repeat(emu, tmp_path):
    for c in Z.multi_block_frames():
        raw = Z.as_is(c.frame, len(c.want))
        assert oracle.zstd_block(raw) == c.want, c.name
        assert run(emu, tmp_path, raw) == c.want, c.name


def test_emulator_damaged_frames(emu, tmp_path):
    cases = Z.damaged(random.Random(6), Z.assembled_forms() + Z.library_frames()[::3], 40)
    for name, f, n in cases:
        raw = Z.as_is(f, n)
        want = oracle.zstd_block(raw)
        got = run(emu, tmp_path, raw)
        assert got == want or (isinstance(want, int) and isinstance(got, int)), name
