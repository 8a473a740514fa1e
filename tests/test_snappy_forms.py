"""Every snappy element form snappy.Decode accepts, on the CPU: the blocks
tests/snappyutil.py assembles (1- to 4-byte literal lengths, non-canonical
literal headers, copies with 1-, 2- and 4-byte offsets at both ends of their
length range, copies of copies, 1-byte copies, element counts around one
round's queue, the route boundaries) are held to the oracle; the corpus the GPU
tests decode (tests/test_snappy_forms_gpu.py) is held to a census floor on each
of the device's three routes, counted by a parser from the blocks' bytes; and
the host emulation of snappy_dec.hip.h (scripts/snappy_emu.cpp: the walked
route, snappy2_kernel's LDS decoder and the one-lane global-memory decoder)
must take the route snappyutil.route() names for every block, decode a sample
chosen by census cell to the oracle's bytes and reject what the oracle rejects.

The emulator replaces the DPP scan and the unaligned global loads and sees no
output placement: those run only in the GPU tests."""
import os
import random
import subprocess

import pytest

import oracle
import snappyutil as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DAMAGE_SEED, DAMAGE_COUNT = 42, 90


def small_cases():
    """The cases damaged() works on: those that take the walked or the LDS route as they are."""
    return [c for c in S.corpus() if len(c.want) <= 8192]


def test_assembler_writes_what_the_parser_reads():
    """One block with every element form, walked back field by field."""
    data = bytes(range(70))
    block, want = S.assemble([S.lit(data[:5]), S.lit(data[:5], 1), S.lit(data, 1), S.lit(data, 2), S.lit(data[:7], 3),
                              S.lit(data, 4), S.c1(200, 11), S.c2(5, 1), S.c4(239, 64), S.c2(64, 64), S.c2(64, 64),
                              S.c2(3, 9)])
    assert block[:2] == S.uvarint(len(want)) and len(want) == 5 + 5 + 70 + 70 + 7 + 70 + 11 + 1 + 64 + 64 + 64 + 9
    D, elems, out = S.parse(block)
    assert (D, out) == (len(want), want) and oracle.snappy_decode(block) == want
    assert [(e.kind, e.form, e.length, e.off) for e in elems] == [
        (0, 0, 5, 0), (0, 1, 5, 0), (0, 1, 70, 0), (0, 2, 70, 0), (0, 3, 7, 0), (0, 4, 70, 0), (1, 0, 11, 200), (2, 0, 1, 5),
        (4, 0, 64, 239), (2, 0, 64, 64), (2, 0, 64, 64), (2, 0, 9, 3)]
    assert [e.depth for e in elems[6:]] == [1, 2, 1, 2, 3, 1]   # (the 9-byte copy overlaps itself)
    assert [e.d for e in elems[:4]] == [0, 5, 10, 80] and [e.s for e in elems[:3]] == [2, 8, 15]
    cen = S.census(block)
    assert {k: cen[k] for k in ("lit_form_0", "lit_form_1", "lit_form_2", "lit_form_3", "lit_form_4", "lit_noncanonical",
                                "copy_1", "copy_2", "copy_4", "copy_len_1_3", "off_lt16", "off_17_up", "off_eq_d",
                                "chain_1", "chain_2_8", "lit_len_lt16", "lit_len_16_256")} == {
        "lit_form_0": 1, "lit_form_1": 2, "lit_form_2": 1, "lit_form_3": 1, "lit_form_4": 1, "lit_noncanonical": 4,
        "copy_1": 1, "copy_2": 4, "copy_4": 1, "copy_len_1_3": 1, "off_lt16": 2, "off_17_up": 3, "off_eq_d": 1,
        "chain_1": 3, "chain_2_8": 3, "lit_len_lt16": 3, "lit_len_16_256": 3}


def test_route_restates_the_constants():
    R = S.route
    assert (R(7, 100), R(8, 100)) == ("lds", "walk") and (R(100, 63), R(100, 64)) == ("lds", "walk")
    assert (R(36864, 32768), R(36865, 32768)) == ("walk", "global") and (R(2000, 32768), R(2000, 32769)) == ("walk", "lds")
    assert (R(32768, 40000), R(32769, 40000)) == ("lds", "global") and (R(2000, 65535), R(2000, 65536)) == ("lds", "global")
    assert S.bitmap_floor(385) == 68 and (R(385, 67), R(385, 68)) == ("lds", "walk")


def test_corpus_decodes_under_the_oracle_on_every_wrapper():
    blocks = S.wrapped_corpus()
    assert 100 <= len(S.corpus()) <= 200 and len(blocks) <= 900
    for w in blocks:
        assert oracle.snappy_decode(w.block) == w.want, (w.name, w.wrapper)
        assert S.route(len(w.block), len(w.want)) == w.route
    # every case reaches the global route; only those with more input than kSnIn, or
    # more output than 65535 bytes, miss the LDS route
    for c in S.corpus():
        routes = {w.route for w in S.wrapped(c)}
        block, want = S.as_is(c)
        assert "global" in routes, c.name
        assert ("lds" in routes) == (len(block) <= S.K_SN_IN and len(want) <= S.LDS_D_MAX), c.name


def test_the_parser_is_a_second_decoder():
    for w in S.wrapped_corpus()[::5]:
        assert S.decode(w.block) == w.want, (w.name, w.wrapper)
    for r in S.rejected():
        assert S.decode(r.block) is None, r.name


def test_corpus_holds_the_boundaries_it_names():
    by = {c.name: S.as_is(c) for c in S.corpus()}
    nD = {k: (len(b), len(w)) for k, (b, w) in by.items()}
    assert nD["edge/n7"][0] == 7 and nD["edge/n8"][0] == 8 and nD["edge/D63"][1] == 63 and nD["edge/D64"][1] == 64
    n, D = nD["edge/D_at_floor"]
    assert D == S.bitmap_floor(n) >= 64 and S.route(n, D) == "walk"
    n, D = nD["edge/D_below_floor"]
    assert D == S.bitmap_floor(n) - 1 >= 64 and S.route(n, D) == "lds"
    assert by["edge/empty"] == (b"\0", b"")
    for D in (32768, 32769, 65535, 65536):
        assert nD["edge/D%d" % D][1] == D
    for n in (32768, 32769, 36864, 36865):
        assert nD["edge/n%d" % n][0] == n
    assert [S.route(*nD["edge/" + k]) for k in ("D32768", "D32769", "D65535", "D65536", "n32768", "n32769", "n36864", "n36865")] \
        == ["walk", "lds", "lds", "global", "lds", "global", "walk", "global"]
    for count in S.ELEMENT_COUNTS:
        for kind in ("lits", "mixed", "big"):
            assert len(S.parse(by["count/%s_%d" % (kind, count)][0])[1]) == count
    for depth in S.CHAIN_DEPTHS:
        for shift in (0, 3):
            assert max(e.depth for e in S.parse(by["chain/depth%d_shift%d" % (depth, shift)][0])[1]) == depth
    # copies from the first output byte at each route's far end, and offsets past 16 bits
    for name, route, top in (("far/walk", "walk", 32340), ("far/lds", "lds", 41393), ("far/global", "global", 66384)):
        elems = S.parse(by[name][0])[1]
        assert S.route(*nD[name]) == route and max(e.off for e in elems) == top
        assert sum(e.off == e.d for e in elems) >= 2, name
    for name in ("onebyte/c4_off1", "onebyte/c2_off1", "onebyte/c4_c2_off5"):
        assert nD[name][0] >= 3 * nD[name][1]


def test_census_floor_on_every_route():
    """A condition, not a measurement: each route sees every literal form,
    copy kind and offset class, the short copies, deep chains, more elements
    than one round holds and, where the route reaches them, elements at output
    offsets that need the high half of the 16-bit fields."""
    cen = S.route_census(S.wrapped_corpus())
    for r in S.ROUTE_NAMES:
        assert [k for k in S.FLOOR[r] if cen[r][k] == 0] == [], (r, sorted(cen[r].items()))
        for cells in (S.LIT_FORMS, S.COPY_KINDS, S.OFF_CLASSES):
            assert set(cells) <= set(S.FLOOR[r])
    assert cen["walk"]["elem_at_32768"] == 0    # (the walked route ends there)
    # the rare forms sit at high offsets too, not only the pad: each route's front-wrapped share
    for r, key in (("lds", "elem_at_32768"), ("global", "elem_at_65536")):
        front = S.route_census([w for w in S.wrapped_corpus() if w.wrapper == "front_" + r])[r]
        assert all(front[k] for k in S.LIT_FORMS + S.COPY_KINDS + ["copy_len_1_3", "chain_gt64", key]), (r, sorted(front.items()))
    # the sample the emulator runs keeps every cell
    smp = S.route_census(S.sample_by_cell(S.wrapped_corpus(), 2))
    for r in S.ROUTE_NAMES:
        assert set(smp[r]) == set(cen[r])


def test_rejected_blocks_are_rejected_by_the_oracle_on_the_route_they_name():
    cases = S.rejected()
    names = {r.name.rsplit("/", 1)[0] for r in cases}
    assert {"offset_0_c1", "offset_d_plus_1_c4", "offset_bit31", "offset_0x10004", "copy_past_D", "literal_past_D",
            "output_short_of_D", "literal_past_input", "copy_before_output", "wrapped_length_first", "wrapped_length_middle",
            "wrapped_length_last", "cut_lit4_4", "cut_c4_4", "cut_c2_2", "cut_c1_1"} <= names
    for r in cases:
        assert oracle.snappy_decode(r.block) is None, r.name
        if r.route is None:
            with pytest.raises(S.Corrupt):
                S.header(r.block)
        else:
            D, _ = S.header(r.block)
            assert S.route(len(r.block), D) == r.route, r.name
    for route in S.ROUTE_NAMES:
        assert sum(r.route == route for r in cases) >= 30


def test_damaged_blocks_decode_and_fail_in_fair_shares():
    cases = S.damaged(random.Random(DAMAGE_SEED), small_cases(), DAMAGE_COUNT)
    assert len(cases) == DAMAGE_COUNT
    good = 0
    for name, block in cases:
        want = oracle.snappy_decode(block)
        assert S.decode(block) == want, name
        good += want is not None
    assert 4 * good >= DAMAGE_COUNT and 4 * (DAMAGE_COUNT - good) >= DAMAGE_COUNT, good


# ---- the host emulation of snappy_dec.hip.h -----------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("semu") / "snappy_emu")
    subprocess.run([CLANG, "-O1", "-std=c++20", "-pthread", os.path.join(ROOT, "scripts", "snappy_emu.cpp"), "-o", exe],
                   check=True)
    return exe


def run(emu, tmp_path, raw):
    """(the route the emulator took, its bytes or None when it reports corrupt)."""
    i, o = tmp_path / "in.bin", tmp_path / "out.bin"
    i.write_bytes(raw)
    r = subprocess.run([emu, str(i), str(o)], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)
    return r.stdout.split()[1], (o.read_bytes() if r.returncode == 0 else None)


def test_route_equals_the_compiled_conditions(emu, tmp_path):
    """route() against sn4_walkable and kSnIn as compiled, for every corpus
    block on every wrapper, every rejected block and a grid round each limit."""
    pairs = [(len(w.block), len(w.want)) for w in S.wrapped_corpus()]
    pairs += [(len(r.block), S.header(r.block)[0]) for r in S.rejected() if r.route]
    edges_n = (0, 1, 7, 8, 9, 31, 32, 33, 385, 32767, 32768, 32769, 36863, 36864, 36865, 70000)
    edges_d = (0, 1, 16, 19, 20, 21, 63, 64, 65, 67, 68, 69, 4623, 4624, 4625, 32767, 32768, 32769, 65535, 65536, 65537, 1 << 20)
    pairs += [(n, d) for n in edges_n for d in edges_d]
    f = tmp_path / "pairs.txt"
    f.write_text("".join("%d %d\n" % p for p in pairs))
    r = subprocess.run([emu, "--routes", str(f)], capture_output=True, text=True, check=True)
    assert r.stdout.split() == [S.route(n, d) for n, d in pairs]
    assert {S.route(n, d) for n, d in pairs} == set(S.ROUTE_NAMES)


def test_emulator_decodes_a_sample_of_every_census_cell_on_all_routes(emu, tmp_path):
    sample = S.sample_by_cell(S.wrapped_corpus(), 2)
    assert 60 <= len(sample) <= 130 and {w.route for w in sample} == set(S.ROUTE_NAMES)
    for w in sample:
        assert oracle.snappy_decode(w.block) == w.want
        assert run(emu, tmp_path, w.block) == (w.route, w.want), (w.name, w.wrapper)


def test_emulator_rejects_what_the_oracle_rejects(emu, tmp_path):
    """Every wrapped-length block, and every third of the others, on the
    route each names.  The global route took a literal of 2^32 bytes for one
    of none (its 32-bit length wrapped to 0) and decoded the rest."""
    cases = S.rejected()
    picked = [r for i, r in enumerate(cases) if "wrapped_length" in r.name or i % 3 == 0]
    assert sum("wrapped_length" in r.name for r in picked) == 11
    for r in picked:
        assert oracle.snappy_decode(r.block) is None
        assert run(emu, tmp_path, r.block) == (r.route or "none", None), r.name


def test_emulator_agrees_with_the_oracle_on_damaged_blocks(emu, tmp_path):
    cases = S.damaged(random.Random(DAMAGE_SEED), small_cases(), DAMAGE_COUNT)[::5]
    for name, block in cases:
        assert run(emu, tmp_path, block)[1] == oracle.snappy_decode(block), name
